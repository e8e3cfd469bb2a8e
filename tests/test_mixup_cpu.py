"""Label smoothing / Mixup / CutMix without a GPU: header, library and lib.py carry the two entry points, their argument checks
answer on the host, ``Mixup.params`` draws what its docstring says, the engine's config handling builds the right criterion, and
the error bound the GPU test holds ``mv_mix_batch`` to is one that torch's own fp32 evaluation stays inside."""
import ctypes
import math
import os
import random
import re
import sys

import pytest
import torch

from conftest import ROOT
from mixup_ref import MIX_LAMS, MIX_SHAPES, lam_pair, mix_inputs, mixup_bound

HEADER = os.path.join(ROOT, "include", "myrtle_vision_hip.h")
OK, SHAPE, ALIGN, UNSUPPORTED = 0, -1, -2, -4
ADDR = 1 << 20                                               # 16-byte aligned, never read: every call below ends at its checks


# ---------------------------------------------------------------- C ABI
def test_header_library_and_lib_py_carry_both_entry_points():
    from myrtle_vision.hip import lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+mv_cross_entropy_soft\s*\(", src) and re.search(r"\bint\s+mv_mix_batch\s*\(", src)
    assert lib.SIGNATURES["mv_cross_entropy_soft"] == ("pppppp" "ii" "ff" "i" "f" "p", ctypes.c_int)
    assert lib.SIGNATURES["mv_mix_batch"] == ("pi" "iiii" "i" "f" "iiii" "p", ctypes.c_int)
    handle = lib.lib()
    assert hasattr(handle, "mv_cross_entropy_soft") and hasattr(handle, "mv_mix_batch")
    assert "mixup.hip" in __import__("myrtle_vision.hip.build", fromlist=["SOURCES"]).SOURCES


def _ce(logits=ADDR, labels=ADDR, loss=ADDR, ws=ADDR, B=4, C=8, lam=1.0, eps=0.0, pair_flip=1):
    from myrtle_vision.hip import lib
    return lib.lib().mv_cross_entropy_soft(logits, labels, loss, ws, None, None, B, C, lam, eps, pair_flip, 1.0, None)


@pytest.mark.parametrize("kw,code", [
    (dict(C=1), SHAPE), (dict(C=0), SHAPE), (dict(B=-1), SHAPE),
    (dict(logits=None), ALIGN), (dict(labels=None), ALIGN), (dict(loss=None), ALIGN), (dict(ws=None), ALIGN),
    (dict(eps=-0.1), UNSUPPORTED), (dict(eps=1.0), UNSUPPORTED), (dict(eps=float("nan")), UNSUPPORTED),
    (dict(lam=-0.01), UNSUPPORTED), (dict(lam=1.01), UNSUPPORTED), (dict(lam=float("nan")), UNSUPPORTED),
    (dict(pair_flip=0, lam=0.5), UNSUPPORTED),
    (dict(B=0), OK), (dict(B=0, pair_flip=0), OK), (dict(B=0, lam=0.3, eps=0.1), OK),
    (dict(B=0, logits=None, labels=None, loss=None, ws=None), OK),                # an empty batch has no storage
    (dict(B=0, C=1), SHAPE), (dict(B=0, lam=2.0), UNSUPPORTED),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_cross_entropy_soft_argument_checks(kw, code):
    assert _ce(**kw) == code


def _mix(x=ADDR, elem=0, B=4, Ch=3, H=8, W=8, mode=0, lam=1.0, box=(0, 0, 0, 0)):
    from myrtle_vision.hip import lib
    return lib.lib().mv_mix_batch(x, elem, B, Ch, H, W, mode, lam, *box, None)


@pytest.mark.parametrize("kw,code", [
    (dict(x=None), ALIGN), (dict(x=ADDR + 4), ALIGN), (dict(elem=7), UNSUPPORTED), (dict(elem=2), UNSUPPORTED),
    (dict(B=-1), SHAPE), (dict(Ch=0), SHAPE), (dict(H=0), SHAPE), (dict(W=0), SHAPE), (dict(mode=2), UNSUPPORTED),
    (dict(lam=1.5), UNSUPPORTED), (dict(lam=-0.5), UNSUPPORTED),
    (dict(mode=1, box=(-1, 2, 0, 2)), SHAPE), (dict(mode=1, box=(3, 2, 0, 2)), SHAPE), (dict(mode=1, box=(0, 9, 0, 2)), SHAPE),
    (dict(mode=1, box=(0, 2, -1, 2)), SHAPE), (dict(mode=1, box=(0, 2, 3, 2)), SHAPE), (dict(mode=1, box=(0, 2, 0, 9)), SHAPE),
    (dict(B=140000, lam=0.5), UNSUPPORTED),                                      # more pairs than the launch grid has rows
    # nothing to do: no launch, success (these return before any kernel, or they could not succeed without a device)
    (dict(lam=1.0), OK), (dict(B=0, lam=0.5), OK), (dict(B=1, lam=0.5), OK),
    (dict(mode=1, box=(3, 3, 2, 5)), OK), (dict(mode=1, box=(1, 4, 2, 2)), OK), (dict(mode=1, elem=1, B=1, box=(0, 8, 0, 8)), OK),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_mix_batch_argument_checks(kw, code):
    assert _mix(**kw) == code


# ---------------------------------------------------------------- Mixup.params
SIZES = [(224, 224), (30, 34), (7, 9)]


def _draws(mixer, H, W, n=2000, seed=99):
    random.seed(seed)
    return [mixer.params(H, W) for _ in range(n)]


@pytest.mark.parametrize("H,W", SIZES)
def test_params_boxes_lie_inside_and_lam_is_the_kept_share(H, W):
    from myrtle_vision.utils.mixup import CUTMIX, MIXUP, Mixup
    draws = _draws(Mixup(mixup_alpha=0.8, cutmix_alpha=1.0), H, W)
    modes = {m for m, _, _ in draws}
    assert modes == {MIXUP, CUTMIX}                                              # both alphas set: both modes occur
    share = sum(m == CUTMIX for m, _, _ in draws) / len(draws)
    assert abs(share - 0.5) < 5 * math.sqrt(0.25 / len(draws))                   # switch_prob 0.5, five standard deviations
    for mode, lam, box in draws:
        assert 0.0 <= lam <= 1.0
        if mode == CUTMIX:
            y0, y1, x0, x1 = box
            assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
            assert lam == 1.0 - (y1 - y0) * (x1 - x0) / (H * W)
        else:
            assert box is None
    assert any(m == CUTMIX and (b[1] - b[0]) * (b[3] - b[2]) > 0 for m, _, b in draws)


def test_params_single_modes_prob_and_seed():
    from myrtle_vision.utils.mixup import CUTMIX, MIXUP, Mixup
    assert {m for m, _, _ in _draws(Mixup(mixup_alpha=0.8), 30, 34)} == {MIXUP}
    assert {m for m, _, _ in _draws(Mixup(cutmix_alpha=1.0), 30, 34)} == {CUTMIX}
    assert all(d == (MIXUP, 1.0, None) for d in _draws(Mixup(0.8, 1.0, prob=0.0), 30, 34))
    assert all(d == (MIXUP, 1.0, None) for d in _draws(Mixup(), 30, 34))         # no alpha: nothing is ever mixed
    half = _draws(Mixup(0.8, 1.0, prob=0.5), 30, 34)
    unmixed = sum(d == (MIXUP, 1.0, None) for d in half) / len(half)
    assert abs(unmixed - 0.5) < 5 * math.sqrt(0.25 / len(half))
    m = Mixup(0.8, 1.0)
    assert _draws(m, 224, 224, seed=5) == _draws(m, 224, 224, seed=5)
    assert _draws(m, 224, 224, seed=5) != _draws(m, 224, 224, seed=6)
    with pytest.raises(ValueError):
        Mixup(mixup_alpha=-1.0)
    with pytest.raises(ValueError):
        Mixup(0.8, prob=1.5)


# ---------------------------------------------------------------- engine: which criterion
def test_engine_without_the_keys_builds_the_plain_criterion(monkeypatch):
    from myrtle_vision import engine
    from myrtle_vision.hip.functional import CrossEntropyLoss
    monkeypatch.delitem(sys.modules, "myrtle_vision.utils.mixup", raising=False)
    for cfg in ({}, {"label_smoothing": 0.0, "mixup_alpha": 0.0, "cutmix_alpha": 0.0, "mixup_prob": 1.0, "mixup_switch_prob": 0.5}):
        criterion, mixer = engine._train_criterion("classification", cfg)
        assert type(criterion) is CrossEntropyLoss and mixer is None
    assert type(engine._train_criterion("segmentation", {})[0]) is CrossEntropyLoss
    assert "myrtle_vision.utils.mixup" not in sys.modules                        # not even imported


def test_engine_with_the_keys_builds_the_soft_criterion_and_the_mixer():
    from myrtle_vision import engine
    from myrtle_vision.hip.functional import SoftTargetCrossEntropy
    from myrtle_vision.utils.mixup import Mixup
    criterion, mixer = engine._train_criterion("classification", {"label_smoothing": 0.1})
    assert type(criterion) is SoftTargetCrossEntropy and criterion.smoothing == 0.1 and mixer is None
    criterion, mixer = engine._train_criterion("classification", {"mixup_alpha": 0.8, "mixup_prob": 0.7, "mixup_switch_prob": 0.2})
    assert type(criterion) is SoftTargetCrossEntropy and criterion.smoothing == 0.0
    assert type(mixer) is Mixup and (mixer.mixup_alpha, mixer.cutmix_alpha, mixer.prob, mixer.switch_prob) == (0.8, 0.0, 0.7, 0.2)
    import json
    cfg = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_base_mixup.json")))
    base = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_base.json")))
    extra = {k: v for k, v in cfg["train_config"].items() if k not in base["train_config"]}
    assert extra == {"label_smoothing": 0.1, "mixup_alpha": 0.8, "cutmix_alpha": 1.0}
    assert {k: v for k, v in cfg["train_config"].items() if k not in extra} == base["train_config"]
    assert cfg["vit_config"] == base["vit_config"]
    criterion, mixer = engine._train_criterion("classification", cfg["train_config"])
    assert criterion.smoothing == 0.1 and (mixer.mixup_alpha, mixer.cutmix_alpha, mixer.prob, mixer.switch_prob) == (0.8, 1.0, 1.0, 0.5)


@pytest.mark.parametrize("key", ["label_smoothing", "mixup_alpha", "cutmix_alpha", "mixup_prob", "mixup_switch_prob"])
@pytest.mark.parametrize("task", ["segmentation", "detection"])
def test_engine_refuses_the_keys_on_another_task(task, key):
    from myrtle_vision import engine
    with pytest.raises(ValueError, match=key):
        engine._train_criterion(task, {key: 0.1})


def test_train_worker_refuses_the_keys_on_segmentation_before_any_work(tmp_path):
    """Through ``train_worker`` itself: the error comes before the device is looked for, so this runs anywhere."""
    import json
    from myrtle_vision.engine import train_worker
    cfg = json.load(open(os.path.join(ROOT, "segmentation", "train_configs", "seg_tiny.json")))
    data = json.load(open(os.path.join(ROOT, "segmentation", "data_configs", "data_config.json")))
    cfg["data_config_path"] = str(tmp_path / "data_config.json")
    json.dump(data, open(cfg["data_config_path"], "w"))
    cfg["train_config"]["mixup_alpha"] = 0.8
    with pytest.raises(ValueError, match="mixup_alpha"):
        train_worker(0, 1, cfg, "segmentation")


# ---------------------------------------------------------------- the Mixup bound, on torch's own fp32 evaluation
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mixup_bound_holds_for_torch_fp32(shape, dtype):
    x = mix_inputs(shape, dtype)
    for lam in MIX_LAMS:
        l, o = lam_pair(lam)
        got = (l * x.float() + o * x.float().flip(0)).to(dtype)                  # two rounded products, one rounded sum, one cast
        exact, bound = mixup_bound(x, lam)
        assert bool(((got.double() - exact).abs() <= bound).all())
