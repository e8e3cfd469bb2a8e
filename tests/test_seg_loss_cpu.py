"""Class weights, label smoothing and Dice on the fused segmentation tail, without a GPU: the reference formulas of
tests/seg_loss_ref.py against ``F.cross_entropy`` and against autograd (fp64), ``SegLoss`` validation, the engine's config handling,
the shipped config, ``MIoU.add_areas``, and the C ABI of the three entry points (bindings and the argument checks, which answer
before any launch)."""
import ctypes
import inspect
import json
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
import seg_loss_ref as ref

HEADER = os.path.join(ROOT, "include", "myrtle_vision_hip.h")
OK, SHAPE, ALIGN, UNSUPPORTED = 0, -1, -2, -4
ADDR = 1 << 20                                               # 16-byte aligned, never read: every call below ends at its checks


def _case(shape, labeling, weights):
    B, C, h, w, H, W, seed = shape
    small = ref.make_small(B, C, h, w, seed)
    y, wts = ref.make_labels(B, C, H, W, seed, labeling)
    return small, y, (wts if weights else None), (B, C, h, w, H, W)


# ---------------------------------------------------------------- the formulas
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("labeling", ["valid", "ignored", "absent_class", "zero_weight_class"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.SHAPE_IDS)
def test_reference_ce_is_torch_cross_entropy(shape, labeling, eps):
    small, y, wts, dims = _case(shape, labeling, True)
    z = ref.upsample(small, *dims, torch.float64)
    got = float(ref.terms(z, y, wts, eps, 0.0, 1.0)["ce"])
    want = float(F.cross_entropy(z, y, weight=wts.double(), label_smoothing=eps))
    assert abs(got - want) <= 1e-13 * max(1.0, abs(want)), (got, want)


def test_reference_nan_rules():
    shape = ref.SHAPES[3]
    for labeling, lam in (("all_zero_weight", 0.0), ("all_zero_weight", 0.5), ("all_ignored", 0.5), ("out_of_range", 0.5)):
        small, y, wts, dims = _case(shape, labeling, True)
        r = ref.reference(small, y, dims, wts, 0.1, lam, 1.0, torch.float64)
        assert math.isnan(r["stats"][0]) and math.isnan(r["stats"][4])
        if labeling == "all_zero_weight":                    # torch's 0/0 without smoothing; zero gradient by the contract
            z = ref.upsample(small, *dims, torch.float64)
            assert math.isnan(float(F.cross_entropy(z, y, weight=wts.double())))
            assert r["stats"][6] == 0.0 and not r["dsmall"].any()
        if labeling == "all_ignored":
            assert r["stats"][5] == 0.0 and r["stats"][2] == 0.0 and not r["dsmall"].any()
        if labeling == "out_of_range":                       # the other pixels' gradient is that of the loss without the bad label
            assert r["stats"][3] == 1.0
            y2 = y.clone()
            y2[y2 == dims[1]] = ref.IGNORE
            r2 = ref.reference(small, y2, dims, wts, 0.1, lam, 1.0, torch.float64)
            assert torch.equal(r["dsmall"], r2["dsmall"]) and math.isfinite(r2["stats"][0])


@pytest.mark.parametrize("option", list(ref.OPTIONS))
@pytest.mark.parametrize("labeling", ["valid", "ignored", "absent_class", "zero_weight_class", "out_of_range"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.SHAPE_IDS)
def test_analytic_gradient_is_autograd_of_the_reference_loss(shape, labeling, option):
    use_w, eps, lam, s = ref.OPTIONS[option]
    small, y, wts, dims = _case(shape, labeling, use_w)
    z = ref.upsample(small, *dims, torch.float64).requires_grad_()
    ref.terms(z, y, wts, eps, lam, s)["loss"].backward()
    dz = ref.analytic_dz(z.detach(), y, wts, eps, lam, s)
    scale = float(z.grad.abs().max())
    assert scale > 0 and float((dz - z.grad).abs().max()) <= 1e-12 * scale
    valid, _ = ref.masks(y, dims[1])
    assert not dz.permute(0, 2, 3, 1)[~valid].any()          # ignored and out-of-range pixels carry no gradient


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.SHAPE_IDS)
def test_inputs_keep_the_argmax_margin(shape):
    """fp64 gap between the two largest logits of every pixel > 1e-3: some 500 times the fp32 interpolation error (2e-6), so the GPU
    test may compare the kernel's arg-max with the fp64 one at every pixel."""
    small, y, wts, dims = _case(shape, "valid", False)
    assert ref.reference(small, y, dims, None, 0.0, 0.0, 1.0, torch.float64)["margin"] > 1e-3


def test_areas_have_the_semantics_of_intersect_and_union():
    from myrtle_vision.utils.miou import MIoU, intersect_and_union
    C = 5
    g = torch.Generator().manual_seed(3)
    pred = torch.randint(0, C, (2, 9, 11), generator=g)
    y = torch.randint(0, C, (2, 9, 11), generator=g)
    y[0, :3] = ref.IGNORE
    y[1, 0, 0] = C                                           # dropped, not clamped
    a = ref.areas(pred, y, C)
    i, u, p, l = intersect_and_union(pred, y, C)
    assert torch.equal(a[0].double(), i) and torch.equal(a[1].double(), p) and torch.equal(a[2].double(), l)
    one, two = MIoU(C, "cpu"), MIoU(C, "cpu")
    for _ in range(2):
        one.add_img(pred, y)
        two.add_areas(a)
    assert torch.equal(one.total_area_intersect, two.total_area_intersect) and torch.equal(one.total_area_union, two.total_area_union)
    assert one.get_miou() == two.get_miou()


# ---------------------------------------------------------------- SegLoss
def test_seg_loss_spec_validates_and_is_immutable():
    from myrtle_vision.hip.functional import SegLoss
    spec = SegLoss([1.0, 0.0, 2.5], 0.1, 0.5, 2.0)
    assert (spec.class_weights, spec.label_smoothing, spec.dice_weight, spec.dice_smooth) == ((1.0, 0.0, 2.5), 0.1, 0.5, 2.0)
    plain = SegLoss()
    assert (plain.class_weights, plain.label_smoothing, plain.dice_weight, plain.dice_smooth) == (None, 0.0, 0.0, 1.0)
    assert plain.weight_on("cpu") is None
    wt = spec.weight_on("cpu")
    assert wt.dtype == torch.float32 and wt.tolist() == [1.0, 0.0, 2.5] and spec.weight_on("cpu") is wt      # uploaded once
    with pytest.raises(AttributeError):
        spec.label_smoothing = 0.2
    assert not callable(spec)
    spec.check_classes(3)
    with pytest.raises(ValueError, match="3 class_weights for 17 classes"):
        spec.check_classes(17)
    for bad in (dict(class_weights=[1.0, -0.5]), dict(class_weights=[1.0, float("nan")]), dict(class_weights=[]),
                dict(label_smoothing=-0.1), dict(label_smoothing=1.0), dict(label_smoothing=float("nan")),
                dict(dice_weight=-1.0), dict(dice_weight=0.5, dice_smooth=0.0), dict(dice_weight=0.5, dice_smooth=-1.0)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            SegLoss(**bad)
    SegLoss(dice_weight=0.0, dice_smooth=0.0)                # the smooth term is only looked at with Dice on


# ---------------------------------------------------------------- engine
CFG = {"class_weights": None, "label_smoothing": 0.1, "dice_weight": 0.5, "dice_smooth": 1.0}


def test_engine_takes_seg_loss_on_segmentation():
    from myrtle_vision import engine
    from myrtle_vision.hip.functional import CrossEntropyLoss, SegLoss
    spec = engine._seg_loss_spec("segmentation", {"seg_loss": dict(CFG, class_weights=[1.0] * 17)}, 17)
    assert type(spec) is SegLoss and spec.class_weights == (1.0,) * 17
    assert (spec.label_smoothing, spec.dice_weight, spec.dice_smooth) == (0.1, 0.5, 1.0)
    assert engine._seg_loss_spec("segmentation", {"seg_loss": {}}, 17).dice_weight == 0.0
    with pytest.raises(ValueError, match="class_weights"):
        engine._seg_loss_spec("segmentation", {"seg_loss": dict(CFG, class_weights=[1.0] * 16)}, 17)
    with pytest.raises(ValueError, match="seg_loss"):
        engine._seg_loss_spec("segmentation", {"seg_loss": {"focal_gamma": 2.0}}, 17)
    # the training criterion next to it stays the plain one (validation's): the recipe lives in the spec alone
    assert type(engine._train_criterion("segmentation", {"seg_loss": CFG})[0]) is CrossEntropyLoss


def test_engine_without_the_key_changes_nothing():
    from myrtle_vision import engine
    from myrtle_vision.hip.functional import CrossEntropyLoss
    for task in ("classification", "segmentation", "detection"):
        assert engine._seg_loss_spec(task, {}) is None
    criterion, mixer = engine._train_criterion("segmentation", {})
    assert type(criterion) is CrossEntropyLoss and mixer is None and engine._fused_seg_tail("segmentation", criterion)


@pytest.mark.parametrize("task", ["classification", "detection"])
def test_engine_refuses_seg_loss_on_another_task(task):
    from myrtle_vision import engine
    with pytest.raises(ValueError, match="seg_loss"):
        engine._seg_loss_spec(task, {"seg_loss": CFG})


def test_engine_keeps_refusing_top_level_label_smoothing_on_segmentation():
    from myrtle_vision import engine
    with pytest.raises(ValueError, match="label_smoothing"):
        engine._train_criterion("segmentation", {"label_smoothing": 0.1, "seg_loss": CFG})


@pytest.mark.parametrize("task,folder,name", [("classification", "classification", "vit_tiny.json"),
                                               ("detection", "detection", "yolos_tiny.json")])
def test_train_worker_refuses_seg_loss_before_any_device_work(tmp_path, monkeypatch, task, folder, name):
    """Through ``train_worker`` itself: the error comes before the device is looked for, so this runs anywhere."""
    from myrtle_vision import engine
    cfg = json.load(open(os.path.join(ROOT, folder, "train_configs", name)))
    data = json.load(open(os.path.join(ROOT, folder, "data_configs", "data_config.json")))
    cfg["data_config_path"] = str(tmp_path / "data_config.json")
    json.dump(data, open(cfg["data_config_path"], "w"))
    cfg["train_config"]["seg_loss"] = CFG
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was looked for first"))
    with pytest.raises(ValueError, match="seg_loss"):
        engine.train_worker(0, 1, cfg, task)


def test_shipped_config_is_seg_base_plus_the_recipe():
    from myrtle_vision import engine
    cfg = json.load(open(os.path.join(ROOT, "segmentation", "train_configs", "seg_base_dice.json")))
    base = json.load(open(os.path.join(ROOT, "segmentation", "train_configs", "seg_base.json")))
    extra = {k: v for k, v in cfg["train_config"].items() if k not in base["train_config"]}
    assert extra == {"seg_loss": CFG}
    assert {k: v for k, v in cfg["train_config"].items() if k not in extra} == base["train_config"]
    assert {k: v for k, v in cfg.items() if k != "train_config"} == {k: v for k, v in base.items() if k != "train_config"}
    data = json.load(open(os.path.join(ROOT, "segmentation", "data_configs", "data_config.json")))
    spec = engine._seg_loss_spec("segmentation", cfg["train_config"], data["number_of_classes"])
    assert (spec.class_weights, spec.label_smoothing, spec.dice_weight, spec.dice_smooth) == (None, 0.1, 0.5, 1.0)


# ---------------------------------------------------------------- model interface
def test_segmentation_loss_still_accepts_img_and_labels():
    from myrtle_vision.models.vit import SegmentationDecoder, ViT
    sig = inspect.signature(ViT.segmentation_loss)
    sig.bind(None, "img", "labels")                          # bench.py's call
    assert [p.name for p in sig.parameters.values()] == ["self", "img", "labels", "loss", "return_areas"]
    assert sig.parameters["loss"].default is None and sig.parameters["return_areas"].default is False
    assert inspect.signature(SegmentationDecoder.loss).parameters["loss"].default is None


def test_a_recipe_outside_the_fused_tail_is_an_error_that_names_the_limit():
    from myrtle_vision.models.vit import SegmentationDecoder
    from myrtle_vision.hip import ops
    labels = torch.zeros(1, 64, 64, dtype=torch.int64)
    SegmentationDecoder(64, 5, 64, 16).require_recipe_tail(labels)
    with pytest.raises(ValueError, match="33 classes exceed its limit of 32"):
        SegmentationDecoder(64, 33, 64, 16).require_recipe_tail(labels)
    with pytest.raises(ValueError, match="KB of LDS"):
        SegmentationDecoder(64, 17, 640, 16).require_recipe_tail(torch.zeros(1, 640, 640, dtype=torch.int64))
    dec = SegmentationDecoder(64, 5, 64, 16)
    dec.linear = torch.nn.Sequential(torch.nn.Identity(), dec.linear)        # what prepare_qat makes of it
    with pytest.raises(ValueError, match="quantiser"):
        dec.require_recipe_tail(labels)
    assert ops.seg_loss_supported(17, 14, 14, 224) and ops.seg_loss_supported(17, 16, 16, 256) and ops.seg_loss_supported(32, 2, 2, 257)
    assert not ops.seg_loss_supported(33, 14, 14, 224) and not ops.seg_loss_supported(17, 40, 40, 640)


# ---------------------------------------------------------------- C ABI
def test_header_library_and_lib_py_carry_the_entry_points():
    from myrtle_vision.hip import lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\blong\s+mv_seg_loss_partials\s*\(", src)
    assert re.search(r"\bint\s+mv_seg_loss_fwd\s*\(", src) and re.search(r"\bint\s+mv_seg_loss_bwd\s*\(", src)
    assert lib.SIGNATURES["mv_seg_loss_partials"] == ("iiii", ctypes.c_long)
    assert lib.SIGNATURES["mv_seg_loss_fwd"] == ("ppp" "fff" "pppppp" "iiiiii" "p", ctypes.c_int)
    assert lib.SIGNATURES["mv_seg_loss_bwd"] == ("ppp" "ff" "pppp" "ii" "f" "iiiiii" "p", ctypes.c_int)
    handle = lib.lib()
    assert "seg_loss.hip" in __import__("myrtle_vision.hip.build", fromlist=["SOURCES"]).SOURCES
    # one row of 4 + 5C words per forward block of 1024 pixels
    assert handle.mv_seg_loss_partials(256, 17, 224, 224) == 256 * 49 * (4 + 5 * 17)
    assert handle.mv_seg_loss_partials(3, 17, 33, 35) == 3 * 2 * 89
    assert handle.mv_seg_loss_partials(0, 17, 224, 224) == 0


def test_seg_tail_kernels_moved_only_their_helpers():
    csrc = os.path.join(ROOT, "myrtle-vision_amd", "csrc")
    tail, loss = open(os.path.join(csrc, "seg_tail.hip")).read(), open(os.path.join(csrc, "seg_loss.hip")).read()
    common = open(os.path.join(csrc, "seg_common.h")).read()
    for helper in ("seg_src", "seg_interp", "seg_stage_map"):
        assert re.search(rf"__device__ __forceinline__ \w+ {helper}\(", common)
        assert not re.search(rf"__device__ __forceinline__ \w+ {helper}\(", tail + loss)
    assert '#include "seg_common.h"' in tail and '#include "seg_common.h"' in loss


def _fwd(small=ADDR, B=2, C=17, h=3, w=4, H=33, W=35, eps=0.0, lam=0.0, s=1.0):
    from myrtle_vision.hip import lib
    return lib.lib().mv_seg_loss_fwd(small, ADDR, None, eps, lam, s, ADDR, ADDR, ADDR, ADDR, ADDR, None, B, C, h, w, H, W, None)


def _bwd(B=2, C=17, h=3, w=4, H=33, W=35, eps=0.0, lam=0.0, elem=0, ld=None):
    from myrtle_vision.hip import lib
    return lib.lib().mv_seg_loss_bwd(ADDR, ADDR, None, eps, lam, ADDR, ADDR, ADDR, ADDR, elem, C if ld is None else ld, 1.0,
                                     B, C, h, w, H, W, None)


@pytest.mark.parametrize("kw,code", [
    (dict(C=33), UNSUPPORTED), (dict(C=0), SHAPE), (dict(B=-1), SHAPE), (dict(B=65536), SHAPE), (dict(h=0), SHAPE), (dict(w=0), SHAPE),
    (dict(H=0), SHAPE), (dict(W=-3), SHAPE), (dict(C=17, h=40, w=40, H=640, W=640), UNSUPPORTED),
    (dict(eps=-0.1), UNSUPPORTED), (dict(eps=1.0), UNSUPPORTED), (dict(eps=float("nan")), UNSUPPORTED),
    (dict(lam=-0.5), UNSUPPORTED), (dict(lam=float("nan")), UNSUPPORTED), (dict(lam=0.5, s=0.0), UNSUPPORTED),
    (dict(lam=0.5, s=-1.0), UNSUPPORTED), (dict(lam=0.5, s=float("nan")), UNSUPPORTED),
    (dict(B=0, C=33), UNSUPPORTED), (dict(B=0, eps=1.5), UNSUPPORTED),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_seg_loss_fwd_argument_checks(kw, code):
    """Every code is answered on the host, before any launch (the addresses are never read; there is no device here)."""
    assert _fwd(**kw) == code


@pytest.mark.parametrize("kw,code", [
    (dict(C=33, ld=40), UNSUPPORTED), (dict(C=0), SHAPE), (dict(B=-1), SHAPE), (dict(B=65536), SHAPE), (dict(h=0), SHAPE),
    (dict(ld=16), SHAPE), (dict(elem=2), UNSUPPORTED), (dict(elem=7), UNSUPPORTED),
    (dict(C=17, h=32, w=32, H=512, W=512), UNSUPPORTED), (dict(C=32, h=2, w=2, H=5, W=600), UNSUPPORTED),
    (dict(eps=1.0), UNSUPPORTED), (dict(eps=-0.1), UNSUPPORTED), (dict(lam=-0.5), UNSUPPORTED),
    (dict(B=0), OK), (dict(B=0, lam=0.5, eps=0.1, elem=1, ld=24), OK),                      # an empty batch: nothing to write
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_seg_loss_bwd_argument_checks(kw, code):
    assert _bwd(**kw) == code
