"""SGD, momentum and LAMB on the one-launch table step without a GPU: the C ABI of ``mv_sgd_table`` / ``mv_lamb_table`` (header,
``SIGNATURES``, export, argument checks answered on the host), ``create_optimizer``'s dispatch, the per-item tensor tables (as a
property test), the checkpoints of each kind and the shipped config."""
import argparse
import ctypes
import json
import os
import random
import re

import pytest
import torch

from conftest import ROOT
from optim_family_ref import EDGE_SIZES, ITEM_MAX, arena_offsets

HEADER = os.path.join(ROOT, "include", "myrtle_vision_hip.h")
OK, SHAPE, ALIGN, UNSUPPORTED = 0, -1, -2, -4
ADDR = 1 << 20                                               # 16-byte aligned, never read: every call below ends at its checks


def _vit(depth=2):
    from myrtle_vision.models.vit import ViT
    return ViT(image_size=224, patch_size=16, dim=64, depth=depth, heads=1, mlp_dim=128, decoder="classification", num_classes=5)


def _args(**extra):
    from myrtle_vision.utils.models import get_optimizer_args
    cfg = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_tiny.json")))["train_config"]
    cfg.update(extra)
    return get_optimizer_args(cfg)


# ---------------------------------------------------------------- C ABI
def test_header_signatures_and_library_carry_the_entry_points():
    from myrtle_vision.hip import build, lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+mv_sgd_table\s*\(", src) and re.search(r"\bint\s+mv_lamb_table\s*\(", src)
    assert re.search(r"\bsize_t\s+mv_lamb_workspace_bytes\s*\(\s*long\s+n_items\s*\)", src)
    assert lib.SIGNATURES["mv_sgd_table"] == ("pppp" "ppp" "l" "pp" "i" "p" "ff" "i" "f" "p" "f" "p", ctypes.c_int)
    assert lib.SIGNATURES["mv_lamb_workspace_bytes"] == ("l", ctypes.c_size_t)
    assert lib.SIGNATURES["mv_lamb_table"] == ("ppppp" "pppp" "l" "pi" "pp" "i" "p" "fffffff" "p" "f" "pz" "p", ctypes.c_int)
    for name in ("mv_sgd_table", "mv_lamb_workspace_bytes", "mv_lamb_table"):
        assert hasattr(lib.lib(), name)
    assert "optim_family.hip" in build.SOURCES
    assert callable(ops.sgd_table_step) and callable(ops.lamb_table_step)
    assert lib.lib().mv_lamb_workspace_bytes(0) == 0 and lib.lib().mv_lamb_workspace_bytes(21027) == 16 * 21027
    assert lib.lib().mv_lamb_workspace_bytes(-3) == 0


def _sgd(p=ADDR, g=ADDR, buf=ADDR, ema=None, off=ADDR, length=ADDR, seg=ADDR, n_items=4, scale=ADDR, wd=ADDR, n_seg=2, hyper=None,
         mu=0.9, nesterov=0, ema_decay=0.0):
    from myrtle_vision.hip import lib
    return lib.lib().mv_sgd_table(p, g, buf, ema, off, length, seg, n_items, scale, wd, n_seg, hyper, 1e-3, mu, nesterov, 1.0, None,
                                  ema_decay, None)


@pytest.mark.parametrize("kw,code", [
    (dict(p=None), ALIGN), (dict(g=None), ALIGN), (dict(buf=None), ALIGN), (dict(p=ADDR + 4), ALIGN), (dict(g=ADDR + 8), ALIGN),
    (dict(buf=ADDR + 4), ALIGN), (dict(ema=ADDR + 4, ema_decay=0.5), ALIGN),
    (dict(off=None), ALIGN), (dict(length=None), ALIGN), (dict(seg=None), ALIGN), (dict(scale=None), ALIGN), (dict(wd=None), ALIGN),
    (dict(n_items=-1), SHAPE), (dict(n_seg=0), SHAPE), (dict(n_seg=-3), SHAPE), (dict(n_items=0, n_seg=0), SHAPE),
    (dict(mu=1.0), UNSUPPORTED), (dict(mu=-0.1), UNSUPPORTED), (dict(mu=float("nan")), UNSUPPORTED), (dict(mu=1.5, n_items=0), UNSUPPORTED),
    (dict(mu=0.0, nesterov=1), UNSUPPORTED), (dict(mu=0.0, nesterov=1, buf=None), UNSUPPORTED),
    (dict(ema=ADDR, ema_decay=1.0), UNSUPPORTED), (dict(ema=ADDR, ema_decay=-0.1), UNSUPPORTED),
    (dict(ema=ADDR, ema_decay=float("nan")), UNSUPPORTED),
    # nothing to do: success with no launch (these return before any kernel, or they could not succeed without a device)
    (dict(n_items=0), OK), (dict(n_items=0, nesterov=1), OK), (dict(n_items=0, mu=0.0, buf=None), OK),
    (dict(n_items=0, ema=ADDR, ema_decay=0.999), OK), (dict(n_items=0, hyper=ADDR), OK),
    (dict(n_items=0, off=None, length=None, seg=None), OK),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_sgd_table_argument_checks(kw, code):
    assert _sgd(**kw) == code


def _lamb(p=ADDR, g=ADDR, m=ADDR, v=ADDR, ema=None, off=ADDR, length=ADDR, seg=ADDR, tensor=ADDR, n_items=4, rng=ADDR, n_tensors=2,
          scale=ADDR, wd=ADDR, n_seg=2, hyper=None, beta1=0.9, beta2=0.999, ema_decay=0.0, ws=ADDR, ws_bytes=64):
    from myrtle_vision.hip import lib
    return lib.lib().mv_lamb_table(p, g, m, v, ema, off, length, seg, tensor, n_items, rng, n_tensors, scale, wd, n_seg, hyper, 1e-3,
                                   beta1, beta2, 1e-6, 0.1, 0.001, 1.0, None, ema_decay, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,code", [
    (dict(p=None), ALIGN), (dict(g=None), ALIGN), (dict(m=None), ALIGN), (dict(v=None), ALIGN),
    (dict(p=ADDR + 4), ALIGN), (dict(g=ADDR + 8), ALIGN), (dict(m=ADDR + 4), ALIGN), (dict(v=ADDR + 12), ALIGN),
    (dict(ema=ADDR + 4, ema_decay=0.5), ALIGN),
    (dict(off=None), ALIGN), (dict(length=None), ALIGN), (dict(seg=None), ALIGN), (dict(tensor=None), ALIGN), (dict(rng=None), ALIGN),
    (dict(scale=None), ALIGN), (dict(wd=None), ALIGN),
    (dict(ws=None), ALIGN), (dict(ws=ADDR + 8), ALIGN), (dict(ws_bytes=63), ALIGN), (dict(ws_bytes=0), ALIGN),
    (dict(n_items=-1), SHAPE), (dict(n_seg=0), SHAPE), (dict(n_tensors=-1), SHAPE), (dict(n_tensors=0), SHAPE),
    (dict(n_items=0, n_seg=0), SHAPE),
    (dict(beta1=1.0), UNSUPPORTED), (dict(beta1=-0.1), UNSUPPORTED), (dict(beta2=1.0), UNSUPPORTED), (dict(beta2=-0.5), UNSUPPORTED),
    (dict(beta1=float("nan")), UNSUPPORTED), (dict(beta2=float("nan")), UNSUPPORTED),
    (dict(ema=ADDR, ema_decay=1.0), UNSUPPORTED), (dict(ema=ADDR, ema_decay=float("nan")), UNSUPPORTED),
    (dict(beta2=1.5, n_items=0), UNSUPPORTED),
    # nothing to do: success with no launch
    (dict(n_items=0), OK), (dict(n_items=0, n_tensors=0), OK), (dict(n_items=0, ws=None, ws_bytes=0), OK),
    (dict(n_items=0, ema=ADDR, ema_decay=0.999), OK), (dict(n_items=0, hyper=ADDR), OK),
    (dict(n_items=0, off=None, length=None, seg=None, tensor=None, rng=None), OK),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_lamb_table_argument_checks(kw, code):
    assert _lamb(**kw) == code


# ---------------------------------------------------------------- create_optimizer
def test_create_optimizer_builds_each_kind():
    """The test that fails without the feature: anything but "adamw" raised NotImplementedError."""
    from myrtle_vision.utils.optim import AdamW, TableAdamW, TableLamb, TableSGD, create_optimizer
    sgd = create_optimizer(_args(optimizer="sgd", momentum=0.8), _vit())
    assert type(sgd) is TableSGD and isinstance(sgd, TableAdamW) and sgd.kind == "sgd"
    assert sgd.nesterov is True and sgd.momentum == 0.8                         # timm: "sgd" is Nesterov
    assert sgd.momentum_buffer.shape == sgd.arena.flat_param.shape and not sgd.momentum_buffer.any()
    assert not hasattr(sgd, "exp_avg") and not hasattr(sgd, "exp_avg_sq")       # ONE state array
    assert sgd.ema is None and [g["name"] for g in sgd.param_groups] == ["decay", "no_decay"]
    assert [g["weight_decay"] for g in sgd.param_groups] == [0.05, 0.0]
    mom = create_optimizer(_args(optimizer="momentum"), _vit())
    assert type(mom) is TableSGD and mom.nesterov is False and mom.momentum == 0.9
    plain = create_optimizer(_args(optimizer="momentum", momentum=0.0), _vit())
    assert plain.momentum_buffer is None                                        # no momentum, no buffer
    lamb = create_optimizer(_args(optimizer="LAMB", opt_eps=None), _vit())      # names are case-insensitive, as "adamw" is
    assert type(lamb) is TableLamb and isinstance(lamb, TableAdamW) and lamb.kind == "lamb"
    assert lamb.defaults["betas"] == (0.9, 0.999) and lamb.defaults["eps"] == 1e-6
    assert create_optimizer(_args(optimizer="lamb"), _vit()).defaults["eps"] == 1e-8       # vit_tiny.json's opt_eps
    assert create_optimizer(_args(optimizer="lamb", opt_betas=[0.8, 0.95]), _vit()).defaults["betas"] == (0.8, 0.95)
    n_items = lamb.items[0].numel()
    assert lamb.item_tensor.dtype == torch.int32 and lamb.item_tensor.numel() == n_items
    assert lamb.tensor_range.dtype == torch.int32 and tuple(lamb.tensor_range.shape) == (len(lamb.arena.params), 2)
    assert lamb.workspace.dtype == torch.float64 and lamb.workspace.numel() >= 2 * n_items
    ws = lamb.workspace
    lamb.param_groups[0]["weight_decay"] = 0.1                                  # the work list is rebuilt, the workspace is not
    lamb._refresh_tables()
    assert lamb.workspace is ws and lamb.segments != create_optimizer(_args(optimizer="lamb"), _vit()).segments
    # the three recipe keys work with every kind
    for name in ("sgd", "momentum", "lamb"):
        opt = create_optimizer(_args(optimizer=name, layer_decay=0.75, no_weight_decay=["pos_embedding"], model_ema_decay=0.99), _vit())
        assert opt.layer_decay == 0.75 and opt.no_weight_decay == ("pos_embedding",) and opt.ema_decay == 0.99
        assert torch.equal(opt.ema, opt.arena.flat_param) and len(opt.segments) > 2
    # "adamw" is what it was
    adamw = create_optimizer(_args(), _vit())
    assert type(adamw) is AdamW and adamw.kind == "adamw"
    for attr in ("items", "seg_lr_scale", "seg_wd", "lr_scales", "item_tensor", "workspace", "momentum_buffer"):
        assert not hasattr(adamw, attr), attr
    assert type(create_optimizer(_args(layer_decay=0.75), _vit())) is TableAdamW


def test_unknown_optimizer_raises_and_lists_the_implemented_ones():
    from myrtle_vision.utils.optim import create_optimizer
    with pytest.raises(NotImplementedError) as e:
        create_optimizer(_args(optimizer="lars"), _vit())
    for name in ("'lars'", "'adamw'", "'sgd'", "'momentum'", "'lamb'"):
        assert name in str(e.value)
    with pytest.raises(ValueError, match="momentum"):
        create_optimizer(_args(optimizer="sgd", momentum=0.0), _vit())          # Nesterov needs momentum, as in torch
    with pytest.raises(ValueError, match="momentum"):
        create_optimizer(_args(optimizer="momentum", momentum=1.0), _vit())


def test_lamb_max_grad_norm_default_null_and_min_with_clip_grad():
    from myrtle_vision.utils.optim import create_optimizer
    assert _args(optimizer="lamb").lamb_max_grad_norm == 1.0                    # absent -> timm's default
    assert _args(optimizer="lamb", lamb_max_grad_norm=None).lamb_max_grad_norm is None
    opt = create_optimizer(_args(optimizer="lamb"), _vit())
    assert opt.lamb_max_grad_norm == 1.0 and opt.max_grad_norm is None and opt._clip_norm() == 1.0
    opt.max_grad_norm = 0.25                                                    # clip_grad below it: one clip, to the smaller
    assert opt._clip_norm() == 0.25
    opt.max_grad_norm = 3.0
    assert opt._clip_norm() == 1.0
    off = create_optimizer(_args(optimizer="lamb", lamb_max_grad_norm=None), _vit())
    assert off.lamb_max_grad_norm is None and off._clip_norm() is None
    off.max_grad_norm = 3.0
    assert off._clip_norm() == 3.0
    assert create_optimizer(_args(optimizer="lamb", lamb_max_grad_norm=0.5), _vit())._clip_norm() == 0.5
    for bad in (0.0, -1.0, "1.0", True, float("nan")):
        with pytest.raises(ValueError, match="lamb_max_grad_norm"):
            create_optimizer(_args(optimizer="lamb", lamb_max_grad_norm=bad), _vit())
    # the other kinds clip to clip_grad alone
    sgd = create_optimizer(_args(optimizer="sgd"), _vit())
    assert sgd._clip_norm() is None
    sgd.max_grad_norm = 2.0
    assert sgd._clip_norm() == 2.0


class _Calls(list):
    pass


@pytest.fixture
def rec(monkeypatch):
    from myrtle_vision.hip import ops
    out = _Calls()
    out.clip_out = torch.tensor([3.0, 0.125])

    def recorder(name, result=None):
        def f(*args, **kw):
            out.append((name, args, kw))
            return result
        return f
    for name in ("adamw_step", "adamw_table_step", "sgd_table_step", "lamb_table_step"):
        monkeypatch.setattr(ops, name, recorder(name))
    monkeypatch.setattr(ops, "grad_norm_clip", recorder("grad_norm_clip", out.clip_out))
    return out


def test_steps_launch_their_own_kernel_through_the_shared_frame(rec):
    from myrtle_vision.utils.optim import create_optimizer
    sgd = create_optimizer(_args(optimizer="sgd", model_ema_decay=0.9), _vit())
    sgd.grad_scale = 0.5
    sgd.step()
    (name, args, kw), = rec
    a = sgd.arena
    assert name == "sgd_table_step" and sgd.step_count == 1
    assert args[0] is a.flat_param and args[1] is a.flat_grad and args[2] is sgd.momentum_buffer and args[3] is sgd.items
    assert args[4] is sgd.seg_lr_scale and args[5] is sgd.seg_wd and len(args) == 6
    assert kw == dict(lr=sgd.param_groups[0]["lr"], momentum=0.9, nesterov=True, grad_scale=0.5, clip_coef=None, hyper=None,
                      ema=sgd.ema, ema_decay=0.9)
    del rec[:]
    lamb = create_optimizer(_args(optimizer="lamb", clip_grad=0.25), _vit())
    lamb.max_grad_norm = 0.25                                                   # what the loops do with clip_grad
    lamb.step()
    (n0, a0, k0), (n1, a1, k1) = rec
    assert n0 == "grad_norm_clip" and a0[1:] == (0.25, 1.0)                     # ONE clip, to min(clip_grad, lamb_max_grad_norm)
    a = lamb.arena
    assert n1 == "lamb_table_step" and len(a1) == 10
    for got, want in zip(a1, (a.flat_param, a.flat_grad, lamb.exp_avg, lamb.exp_avg_sq, lamb.items, lamb.item_tensor,
                              lamb.tensor_range, lamb.seg_lr_scale, lamb.seg_wd, lamb.workspace)):
        assert got is want
    assert k1.pop("clip_coef").data_ptr() == rec.clip_out[1:2].data_ptr()
    assert k1 == dict(lr=lamb.param_groups[0]["lr"], beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=1.0, hyper=None, ema=None,
                      ema_decay=0.0)


# ---------------------------------------------------------------- the per-item tensor tables, as a property test
def _check_item_tensors(sizes):
    from myrtle_vision.utils.optim import build_item_tensors, build_items
    offsets, total = arena_offsets(sizes)
    off, length, seg, _ = build_items(offsets, sizes, [(1.0, 0.0)] * len(sizes))
    item_tensor, first, count = build_item_tensors(sizes)
    assert len(item_tensor) == len(off) and len(first) == len(count) == len(sizes)
    at = 0
    for t, (o, n) in enumerate(zip(offsets, sizes)):
        assert count[t] == -(-n // ITEM_MAX) and first[t] == at                 # ceil(numel / 4096) items; the ranges tile in order
        for k in range(first[t], first[t] + count[t]):
            assert item_tensor[k] == t                                          # every item of the tensor points at it
            assert o <= off[k] and off[k] + length[k] <= o + n                  # and IS an item of that tensor
        assert sum(length[first[t]:first[t] + count[t]]) == n
        at += count[t]
    assert at == len(off)


def test_item_tensor_tables_tile_the_item_list():
    rng = random.Random(4321)
    must = [1, 3, 5, 8, 4095, 4096, 4097, 2 * 4096 + 5, 256 * 4096 + 1]
    for trial in range(25):
        sizes = must + [rng.choice(EDGE_SIZES + [2, 4, 6, 16, 100, 12289]) for _ in range(rng.randint(0, 30))]
        rng.shuffle(sizes)
        _check_item_tensors(sizes)
    _check_item_tensors([1])
    _check_item_tensors([4096, 4096])


# ---------------------------------------------------------------- checkpoints
KINDS = {"adamw": dict(layer_decay=0.75), "sgd": dict(optimizer="sgd"), "momentum": dict(optimizer="momentum"),
         "lamb": dict(optimizer="lamb")}
KIND_OF = {"adamw": "adamw", "sgd": "sgd", "momentum": "sgd", "lamb": "lamb"}


def _state_arrays(opt):
    return [getattr(opt, n) for n in ("exp_avg", "exp_avg_sq", "momentum_buffer") if getattr(opt, n, None) is not None]


@pytest.mark.parametrize("name", ["sgd", "momentum", "lamb"])
def test_checkpoint_round_trip(name, tmp_path):
    from myrtle_vision.utils.models import load_checkpoint, save_checkpoint
    from myrtle_vision.utils.optim import CosineLRScheduler, create_optimizer
    extra = dict(KINDS[name], model_ema_decay=0.99, no_weight_decay=["cls_token"])
    vit = _vit()
    opt = create_optimizer(_args(**extra), vit)
    for arr in _state_arrays(opt):
        arr.normal_()
    opt.step_count = 5
    opt.ema.add_(0.25)
    sched = CosineLRScheduler(opt, t_initial=10, lr_min=1e-5, warmup_t=2, warmup_lr_init=1e-6)
    sched.step(3)
    sd = opt.state_dict()
    assert sd["kind"] == KIND_OF[name] and sd["no_weight_decay"] == ["cls_token"] and sd["layer_decay"] is None
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.0, 0.05]       # torch's group order
    n_params = len(opt.arena.params)
    assert len(sd["state"]) == n_params and all(isinstance(k, int) for k in sd["state"])      # keyed by timm's parameter index
    if name == "lamb":                                                          # AdamW's layout
        assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][0]["step"] == 5
        assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "initial_lr", "params"}
    else:                                                                       # torch.optim.SGD's
        assert set(sd["state"][0]) == {"momentum_buffer"} and sd["step_count"] == 5
        g0 = sd["param_groups"][0]
        assert g0["momentum"] == 0.9 and g0["dampening"] == 0 and g0["nesterov"] is (name == "sgd") and g0["maximize"] is False
        shapes = {tuple(p.shape) for p in opt.arena.params}
        assert {tuple(e["momentum_buffer"].shape) for e in sd["state"].values()} == shapes
    path = str(tmp_path / "ckpt")
    save_checkpoint(vit, opt, sched, 5, path, model_ema=opt.ema_state_dict(vit))
    vit2 = _vit()
    opt2 = create_optimizer(_args(**extra), vit2)
    sched2 = CosineLRScheduler(opt2, t_initial=10, lr_min=1e-5, warmup_t=2, warmup_lr_init=1e-6)
    assert load_checkpoint(vit2, opt2, sched2, path) == 5
    assert opt2.step_count == 5 and opt2.ema_loaded and opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
    s1, s2 = sd["state"], opt2.state_dict()["state"]
    for k in s1:
        for field in s1[k]:
            if field != "step":
                assert torch.equal(s1[k][field], s2[k][field]), (k, field)      # (arena padding is not state)
    assert torch.equal(opt2.arena.flat_param, opt.arena.flat_param)


def test_momentum_zero_checkpoint_has_no_state():
    from myrtle_vision.utils.optim import create_optimizer
    opt = create_optimizer(_args(optimizer="momentum", momentum=0.0), _vit())
    opt.step_count = 3
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["kind"] == "sgd" and sd["step_count"] == 3
    opt2 = create_optimizer(_args(optimizer="momentum", momentum=0.0), _vit())
    opt2.load_state_dict(sd)
    assert opt2.step_count == 3 and opt2.momentum_buffer is None


@pytest.mark.parametrize("writer", list(KINDS))
@pytest.mark.parametrize("reader", list(KINDS) + ["plain_adamw"])
def test_cross_kind_load_raises_and_names_both_kinds(writer, reader):
    from myrtle_vision.utils.optim import create_optimizer
    kinds = dict(KINDS, plain_adamw={})
    kind_of = dict(KIND_OF, plain_adamw="adamw")
    src = create_optimizer(_args(**kinds[writer]), _vit())
    for arr in _state_arrays(src):
        arr.normal_()
    src.step_count = 2
    sd = src.state_dict()
    assert ("kind" in sd) == (kind_of[writer] != "adamw")                       # an "adamw" checkpoint stays the format it is
    dst = create_optimizer(_args(**kinds[reader]), _vit())
    if kind_of[writer] == kind_of[reader]:
        if reader == "plain_adamw" or writer == reader or {writer, reader} == {"sgd", "momentum"}:
            dst.load_state_dict(sd)
            assert dst.step_count == 2
        return
    with pytest.raises(ValueError) as e:
        dst.load_state_dict(sd)
    assert repr(kind_of[writer]) in str(e.value) and repr(kind_of[reader]) in str(e.value)


def test_adamw_checkpoint_keys_are_unchanged():
    from myrtle_vision.utils.optim import create_optimizer
    plain = create_optimizer(_args(), _vit())
    plain.step_count = 1
    assert set(plain.state_dict()) == {"state", "param_groups", "param_names"}
    table = create_optimizer(_args(layer_decay=0.75), _vit())
    assert set(table.state_dict()) == {"state", "param_groups", "param_names", "layer_decay", "no_weight_decay"}


# ---------------------------------------------------------------- the shipped config
def test_shipped_lamb_config_parses():
    from myrtle_vision.utils.models import get_optimizer_args
    d = os.path.join(ROOT, "classification", "train_configs")
    cfg, base = json.load(open(os.path.join(d, "vit_base_lamb.json"))), json.load(open(os.path.join(d, "vit_base_mixup.json")))
    changed = {k for k, v in cfg["train_config"].items() if base["train_config"].get(k, "<absent>") != v}
    assert changed == {"optimizer", "lr", "global_batch_size"}
    assert set(cfg["train_config"]) == set(base["train_config"]) and cfg["vit_config"] == base["vit_config"]
    t = cfg["train_config"]
    assert t["optimizer"] == "lamb" and t["lr"] > base["train_config"]["lr"]
    assert t["global_batch_size"] > base["train_config"]["global_batch_size"] and t["global_batch_size"] % t["local_batch_size"] == 0
    args = get_optimizer_args(t)
    assert args.opt == "lamb" and args.lamb_max_grad_norm == 1.0 and args.momentum == 0.9
    assert isinstance(args, argparse.Namespace)
