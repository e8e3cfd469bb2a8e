"""DeiT distillation without a GPU: the model factory on a ``distiller_config``, the classes' state-dict and parameter-name format,
the frozen teacher, the engine's refusals, the shipped configs, the C ABI of ``mv_distill_loss`` (header, ``SIGNATURES``, export,
argument checks answered on the host) and the fp64 oracle the GPU tests hold the kernel to (tests/distill_ref.py) against torch's
fp64 evaluation of the reference expression."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import distill_ref as R

HEADER = os.path.join(ROOT, "include", "myrtle_vision_hip.h")
CFG_DIR = os.path.join(ROOT, "classification", "train_configs")
OK, SHAPE, ALIGN, UNSUPPORTED = 0, -1, -2, -4
ADDR = 1 << 20                                               # never read: every call below ends at its checks

SMALL = dict(decoder="classification", image_size=80, patch_size=16, embed_dim=128, depth=2, heads=2, mlp_dim=256, dropout=0.0,
             emb_dropout=0.0, q_format="FP32")
TEACHER = dict(SMALL, depth=1)
KW = dict(decoder="classification", image_size=80, patch_size=16, num_classes=45, dim=128, depth=2, heads=2, mlp_dim=256)


def _config(tmp_path, save_teacher=True, wrap=False, **distiller):
    """A small config with a ViT teacher whose state dict (or checkpoint, ``wrap``) is written to ``tmp_path``."""
    from myrtle_vision.models.vit import ViT
    path = str(tmp_path / "teacher.pt")
    if save_teacher:
        sd = ViT(**dict(KW, depth=1)).state_dict()
        torch.save({"model": sd, "iteration": 7} if wrap else sd, path)
    dc = dict(temperature=3, alpha=0.5, teacher_vit_config=dict(TEACHER), teacher_weights_path=path)
    dc.update(distiller)
    return {"vit_config": dict(SMALL), "distiller_config": dc, "train_config": {},
            "data_config_path": os.path.join(ROOT, "classification", "data_configs", "data_config.json")}


# ---------------------------------------------------------------- the factory
@pytest.mark.parametrize("wrap", [False, True], ids=["state_dict", "checkpoint"])
def test_get_models_builds_student_and_wrapper(tmp_path, wrap):
    """The test that fails without the feature: ``get_models`` raised NotImplementedError on a ``distiller_config``."""
    from myrtle_vision.models.distill import DistillableViT, DistillWrapper
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.models import get_models
    cfg = _config(tmp_path, wrap=wrap, distillation_type="hard")
    vit, distiller = get_models(cfg)
    assert type(vit) is DistillableViT and type(distiller) is DistillWrapper and distiller.student is vit
    assert type(distiller.teacher) is ViT and len(distiller.teacher.transformer.layers) == 1
    assert (distiller.temperature, distiller.alpha, distiller.distillation_type) == (3, 0.5, "hard")
    saved = torch.load(cfg["distiller_config"]["teacher_weights_path"], weights_only=False)
    saved = saved["model"] if wrap else saved
    assert all(torch.equal(v, saved[k]) for k, v in distiller.teacher.state_dict().items())
    del cfg["distiller_config"]["distillation_type"]
    assert get_models(cfg)[1].distillation_type == "soft"                   # the reference's loss is the default


def test_with_teacher_false_needs_no_teacher_file(tmp_path):
    from myrtle_vision.models.distill import DistillableViT
    from myrtle_vision.utils.models import get_models
    vit, distiller = get_models(_config(tmp_path, save_teacher=False), with_teacher=False)
    assert type(vit) is DistillableViT and distiller is None


def test_missing_teacher_file_names_the_key(tmp_path):
    from myrtle_vision.utils.models import get_models
    with pytest.raises(FileNotFoundError, match="teacher_weights_path"):
        get_models(_config(tmp_path, save_teacher=False))


def test_unknown_distiller_key_and_type_raise(tmp_path):
    from myrtle_vision.utils.models import get_models
    with pytest.raises(ValueError, match="temperatur"):
        get_models(_config(tmp_path, temperatur=2))
    with pytest.raises(ValueError, match="distillation_type"):
        get_models(_config(tmp_path, distillation_type="medium"))


def test_get_teacher_without_torchvision_names_the_alternative():
    try:
        import torchvision  # noqa: F401
    except ImportError:
        pass
    else:
        pytest.skip("torchvision is installed: get_teacher builds the reference's ResNet-50")
    from myrtle_vision.utils.models import get_teacher
    with pytest.raises(ImportError, match="torchvision") as e:
        get_teacher(45, "nowhere.pth")
    assert "teacher_vit_config" in str(e.value)


# ---------------------------------------------------------------- classes: format, frozen teacher
def test_distillable_vit_has_the_state_dict_of_a_vit_and_converts_strictly():
    from myrtle_vision.models.distill import DistillableViT
    from myrtle_vision.models.vit import ViT
    torch.manual_seed(3)
    plain = ViT(**KW)
    torch.manual_seed(3)
    student = DistillableViT(**KW)
    sa, sb = plain.state_dict(), student.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert (student.dim, student.num_classes, student.args, student.kwargs) == (128, 45, (), KW)
    back = student.to_vit()
    assert type(back) is ViT and all(torch.equal(v, sb[k]) for k, v in back.state_dict().items())
    assert plain.load_state_dict(sb, strict=True).missing_keys == []
    for decoder in ("segmentation", "detection"):
        with pytest.raises(ValueError, match="classification-only"):
            DistillableViT(**dict(KW, decoder=decoder))


def _wrapper(**kw):
    from myrtle_vision.models.distill import DistillableViT, DistillWrapper
    from myrtle_vision.models.vit import ViT
    return DistillWrapper(teacher=ViT(**dict(KW, depth=1)), student=DistillableViT(**KW), **kw)


def test_wrapper_parameter_names_and_frozen_teacher():
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.optim import ParamArena
    w = _wrapper(temperature=3.0, alpha=0.25)
    names = [n for n, _ in w.named_parameters()]
    vit_names = [n for n, _ in ViT(**KW).named_parameters()]
    teacher_names = [n for n, _ in ViT(**dict(KW, depth=1)).named_parameters()]
    head = ["distillation_token", "distill_mlp.0.weight", "distill_mlp.0.bias", "distill_mlp.1.weight", "distill_mlp.1.bias"]
    assert sorted(names) == sorted(head + ["student." + n for n in vit_names] + ["teacher." + n for n in teacher_names])
    assert {n: tuple(p.shape) for n, p in w.named_parameters() if n in head} == {
        "distillation_token": (1, 1, 128), "distill_mlp.0.weight": (128,), "distill_mlp.0.bias": (128,),
        "distill_mlp.1.weight": (45, 128), "distill_mlp.1.bias": (45,)}
    assert all(p.requires_grad != n.startswith("teacher.") for n, p in w.named_parameters())
    assert w.unused_parameter_names() == ("student.pos_embedding_det", "student.det_tokens")
    arena = ParamArena(w.named_parameters(), skip=w.unused_parameter_names())
    assert not any(n.startswith("teacher.") for n in arena.names)
    assert set(arena.names) == set(head + ["student." + n for n in vit_names]) - set(w.unused_parameter_names())
    w.train()
    assert w.training and w.student.training and w.distill_mlp.training and not w.teacher.training
    assert not any(m.training for m in w.teacher.modules())
    w.eval()
    w.train(True)
    assert not w.teacher.training
    with pytest.raises(ValueError, match="distillation_type"):
        _wrapper(distillation_type="firm")
    with pytest.raises(AssertionError, match="vision transformer"):
        from myrtle_vision.models.distill import DistillWrapper
        DistillWrapper(teacher=ViT(**KW), student=ViT(**KW))


def test_cpu_forward_fails_loudly():
    w = _wrapper()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w(torch.randn(2, 3, 80, 80), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.student(torch.randn(2, 3, 80, 80), w.distillation_token)


def test_checkpoint_carries_the_head_and_a_reference_checkpoint_warns(tmp_path, capsys):
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.models import load_checkpoint, save_checkpoint

    class _Stub:
        def state_dict(self):
            return {"stub": 1}

        def load_state_dict(self, sd):
            assert sd == {"stub": 1}

    w = _wrapper()
    path = str(tmp_path / "ck")
    save_checkpoint(w.student, _Stub(), _Stub(), 5, path, distiller=w)
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "iteration", "distiller"}
    assert list(ck["distiller"]) == ["distillation_token", "distill_mlp.0.weight", "distill_mlp.0.bias", "distill_mlp.1.weight",
                                     "distill_mlp.1.bias"]
    assert ViT(**KW).load_state_dict(ck["model"], strict=True).missing_keys == []         # the student's, without a prefix
    other = _wrapper()
    assert not torch.equal(other.distillation_token, w.distillation_token)
    assert load_checkpoint(other.student, _Stub(), _Stub(), path, distiller=other) == 5
    for k, v in w.head_state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    assert "WARNING" not in capsys.readouterr().out
    # a run without a distiller keeps the reference's four keys; resuming a distillation run from it starts a fresh head
    plain = str(tmp_path / "plain")
    save_checkpoint(w.student, _Stub(), _Stub(), 6, plain)
    assert set(torch.load(plain, weights_only=False)) == {"model", "optimizer", "lr_scheduler", "iteration"}
    fresh = _wrapper()
    before = fresh.distillation_token.clone()
    assert load_checkpoint(fresh.student, _Stub(), _Stub(), plain, distiller=fresh) == 6
    assert "no 'distiller' entry" in capsys.readouterr().out and torch.equal(fresh.distillation_token, before)


# ---------------------------------------------------------------- engine: refusals, configs
def _train_config(tmp_path, **extra):
    cfg = json.load(open(os.path.join(CFG_DIR, "deit_tiny.json")))
    cfg["data_config_path"] = os.path.join(ROOT, "classification", "data_configs", "data_config.json")
    cfg["train_config"].update(output_directory=str(tmp_path / "ckpt"), **extra)
    return cfg


@pytest.mark.parametrize("key,value", [("layer_decay", 0.75), ("no_weight_decay", ["cls_token"]), ("model_ema_decay", 0.999)])
def test_train_worker_refuses_the_name_based_keys_before_any_work(tmp_path, key, value):
    from myrtle_vision.engine import train_worker
    with pytest.raises(ValueError, match=key) as e:
        train_worker(0, 1, _train_config(tmp_path, **{key: value}), "classification")
    assert "distiller_config" in str(e.value) and not os.path.exists(str(tmp_path / "ckpt"))


def test_train_worker_refuses_a_quantised_format_and_other_tasks(tmp_path):
    from myrtle_vision.engine import train_worker
    cfg = _train_config(tmp_path)
    cfg["vit_config"]["q_format"] = "FP16_32"
    with pytest.raises(ValueError, match="q_format") as e:
        train_worker(0, 1, cfg, "classification")
    assert "distiller_config" in str(e.value) and "FP16_32" in str(e.value)
    seg = json.load(open(os.path.join(ROOT, "segmentation", "train_configs", "seg_tiny.json")))
    seg["data_config_path"] = os.path.join(ROOT, "segmentation", "data_configs", "data_config.json")
    seg["distiller_config"] = _train_config(tmp_path)["distiller_config"]
    with pytest.raises(ValueError, match="distiller_config"):
        train_worker(0, 1, seg, "segmentation")


def test_graphed_train_step_refuses_a_distiller():
    from myrtle_vision.utils.graph import GraphedTrainStep
    with pytest.raises(ValueError, match="DistillWrapper"):
        GraphedTrainStep(_wrapper(), None, None, torch.zeros(2, 3, 80, 80), torch.zeros(2, dtype=torch.int64))


@pytest.mark.parametrize("size", ["tiny", "small", "base"])
def test_shipped_deit_configs_differ_from_the_vit_configs_in_two_places(size):
    deit = json.load(open(os.path.join(CFG_DIR, f"deit_{size}.json")))
    vit = json.load(open(os.path.join(CFG_DIR, f"vit_{size}.json")))
    base = json.load(open(os.path.join(CFG_DIR, "vit_base.json")))
    dc = deit.pop("distiller_config")
    assert deit["train_config"].pop("output_directory") == f"checkpoints_deit_{size}"
    assert vit["train_config"].pop("output_directory") == f"checkpoints_vit_{size}"
    assert deit == vit
    assert set(dc) == {"temperature", "alpha", "distillation_type", "teacher_vit_config", "teacher_weights_path"}
    assert (dc["temperature"], dc["alpha"], dc["distillation_type"]) == (3, 0.5, "soft")          # the reference's values
    assert dc["teacher_vit_config"] == base["vit_config"] and isinstance(dc["teacher_weights_path"], str)


# ---------------------------------------------------------------- C ABI
def test_header_library_and_lib_py_carry_the_entry_point():
    from myrtle_vision.hip import build, lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+mv_distill_loss\s*\(", src)
    assert "distill.py:142-151" in open(HEADER).read()
    assert lib.SIGNATURES["mv_distill_loss"] == ("ppppppppp" "iii" "ffff" "i" "f" "p", ctypes.c_int)
    assert hasattr(lib.lib(), "mv_distill_loss")
    assert "distill.hip" in build.SOURCES


def _call(student=ADDR, distill=ADDR, teacher=ADDR, labels=ADDR, loss=ADDR, ws=ADDR, B=4, C=8, mode=0, T=1.0, alpha=0.5, lam=1.0,
          eps=0.0, pair_flip=0):
    from myrtle_vision.hip import lib
    return lib.lib().mv_distill_loss(student, distill, teacher, labels, loss, ws, None, None, None, B, C, mode, T, alpha, lam, eps,
                                     pair_flip, 1.0, None)


@pytest.mark.parametrize("kw,code", [
    (dict(C=1), SHAPE), (dict(C=0), SHAPE), (dict(B=-1), SHAPE),
    (dict(T=0.0), UNSUPPORTED), (dict(T=-1.0), UNSUPPORTED), (dict(T=float("nan")), UNSUPPORTED), (dict(T=float("inf")), UNSUPPORTED),
    (dict(alpha=-0.01), UNSUPPORTED), (dict(alpha=1.01), UNSUPPORTED), (dict(alpha=float("nan")), UNSUPPORTED),
    (dict(mode=2), UNSUPPORTED), (dict(mode=-1), UNSUPPORTED),
    (dict(eps=-0.1), UNSUPPORTED), (dict(eps=1.0), UNSUPPORTED), (dict(lam=1.01), UNSUPPORTED), (dict(lam=float("nan")), UNSUPPORTED),
    (dict(pair_flip=0, lam=0.5), UNSUPPORTED),
    (dict(student=None), ALIGN), (dict(distill=None), ALIGN), (dict(teacher=None), ALIGN), (dict(labels=None), ALIGN),
    (dict(loss=None), ALIGN), (dict(ws=None), ALIGN),
    # nothing to do: no launch, success (an empty batch has no storage); the value checks still come first
    (dict(B=0), OK), (dict(B=0, mode=1, alpha=0.0, T=3.0), OK), (dict(B=0, lam=0.3, eps=0.1, pair_flip=1), OK),
    (dict(B=0, student=None, distill=None, teacher=None, labels=None, loss=None, ws=None), OK),
    (dict(B=0, C=1), SHAPE), (dict(B=0, T=0.0), UNSUPPORTED), (dict(B=0, alpha=2.0), UNSUPPORTED),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_distill_loss_argument_checks(kw, code):
    assert _call(**kw) == code


# ---------------------------------------------------------------- the oracle against torch's fp64 evaluation of the reference expression
def _zero_mass_inputs(B, C):
    """As ``distill_ref.inputs`` with p_c == 0 in EVERY row: a teacher logit so low that its weight is exactly 0 in fp64, for both T."""
    s, d, t, y = (v.clone() for v in R.inputs(B, C))
    t[:, 1] = -1.0e4
    return s, d, t, y


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("B,C", [(1, 2), (7, 45), (64, 65), (2, 1001)])
def test_oracle_agrees_with_torch_fp64(B, C, mode):
    for make in (R.inputs, _zero_mass_inputs):
        s, d, t, y = make(B, C)
        assert R.teacher_gap(t) > 0
        if make is _zero_mass_inputs:
            assert bool((torch.softmax(t.double() / 3.0, dim=1) == 0).any(dim=1).all())       # the p_c == 0 branch is taken
        for T in R.TEMPERATURES:
            for alpha in R.ALPHAS:
                for labelling in R.LABELLINGS:
                    ours = R.oracle(s.numpy(), d.numpy(), t.numpy(), y.numpy(), T, alpha, mode, *labelling)
                    ref = R.torch_eval(s, d, t, y, T, alpha, mode, *labelling, dtype=torch.float64)
                    for k in R.QUANTITIES:
                        assert np.all(np.isfinite(ours[k]))
                        assert R.rel_err(ours[k], ref[k]) < 1e-12, (k, T, alpha, labelling)


def test_plain_labelling_is_plain_cross_entropy_and_the_rule_has_no_fixed_number():
    s, d, t, y = R.inputs(7, 45)
    ours = R.oracle(s.numpy(), d.numpy(), t.numpy(), y.numpy(), 1.0, 1.0, "soft")
    assert abs(ours["loss"] - float(torch.nn.functional.cross_entropy(s.double(), y))) < 1e-12
    assert ours["loss"] == ours["ce"] and np.all(ours["ddistill"] == 0)
    assert R.rel_err(np.zeros(3), np.zeros(3)) == 0.0 and R.rel_err(np.array([0.0, 1e-9]), np.zeros(2)) == 1e-9
    assert len(R.settings()) == 24 and R.FACTOR == 8.0
