"""Random Erasing, host side: the C ABI of the two entry points and their host-answered refusals, the constructor, the config keys,
and the statistics of the numpy restatement of the draw and the fill (tests/random_erase_ref.py).  No GPU needed."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest

import random_erase_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "classification", "train_configs")
SEED, STEP = (5 << 40) + 12345, (1 << 32) - 1
OK, ERR_UNSUPPORTED = 0, -4


def test_entry_points_are_declared_bound_and_built():
    from myrtle_vision.hip import build, lib
    assert lib.SIGNATURES["mv_random_erase_draw"] == ("ppp" "iii" "Q" "p" "ii" "p", ctypes.c_int)
    assert lib.SIGNATURES["mv_random_erase_apply"] == ("pipp" "iiii" "ii" "p", ctypes.c_int)
    assert "random_erase.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "myrtle_vision_hip.h")).read()
    for name in ("mv_random_erase_draw", "mv_random_erase_apply"):
        assert f"int {name}(" in header
    assert "timm's RandomErasing" in header and "no call site" in header
    assert '#include "philox.h"' in open(os.path.join(ROOT, "myrtle-vision_amd", "csrc", "random_erase.hip")).read()


def test_argument_checks_are_answered_on_the_host():
    """Before any launch, so these run without a device: nothing to do is MV_OK, a bad dtype / mode / count is refused."""
    from myrtle_vision.hip import lib
    h = lib.lib()
    lo, hi = math.log(0.3), math.log(1 / 0.3)
    fake = 1 << 20                                                       # never dereferenced: every case returns before a launch
    def draw(B=4, thr=1 << 30, a0=0.02, a1=1 / 3, l0=lo, l1=hi, c0=1, c1=1, H=8, W=8, dev=fake):
        area_ratio = (ctypes.c_double * 4)(a0, a1, l0, l1)               # a HOST array: the call reads it before it launches
        return h.mv_random_erase_draw(dev, dev, dev, B, H, W, thr, ctypes.addressof(area_ratio), c0, c1, None)
    assert h.mv_random_erase_draw(None, None, None, 0, 8, 8, 1 << 30, None, 1, 1, None) == OK                     # B == 0
    assert draw(c1=9) == ERR_UNSUPPORTED and draw(c0=3, c1=2) == ERR_UNSUPPORTED and draw(c0=0) == ERR_UNSUPPORTED
    assert draw(thr=(1 << 32) + 1) == ERR_UNSUPPORTED
    assert draw(a0=0.0) == ERR_UNSUPPORTED and draw(a0=0.5, a1=0.4) == ERR_UNSUPPORTED and draw(a1=1.5) == ERR_UNSUPPORTED
    assert draw(a0=float("nan")) == ERR_UNSUPPORTED and draw(l0=hi, l1=lo) == ERR_UNSUPPORTED
    assert draw(l1=float("inf")) == ERR_UNSUPPORTED
    assert draw(B=-1) not in (OK, ERR_UNSUPPORTED) and draw(H=0) not in (OK, ERR_UNSUPPORTED)
    assert draw(dev=None) != OK and h.mv_random_erase_draw(fake, fake, fake, 4, 8, 8, 1 << 30, None, 1, 1, None) != OK   # null arrays
    apply = lambda elem=lib.MV_F32, B=4, mc=1, mode=2, Ch=3: h.mv_random_erase_apply(fake, elem, fake, fake, B, Ch, 8, 8, mc, mode, None)  # noqa: E731
    assert h.mv_random_erase_apply(None, lib.MV_BF16, None, None, 0, 3, 8, 8, 1, 2, None) == OK                   # B == 0
    for elem in (lib.MV_I8, lib.MV_F16, 7):
        assert apply(elem=elem) == ERR_UNSUPPORTED
    assert apply(mc=9) == ERR_UNSUPPORTED and apply(mc=0) == ERR_UNSUPPORTED
    assert apply(mode=3) == ERR_UNSUPPORTED and apply(mode=-1) == ERR_UNSUPPORTED
    assert apply(Ch=0) not in (OK, ERR_UNSUPPORTED)
    assert h.mv_random_erase_apply(None, lib.MV_F32, None, None, 4, 3, 8, 8, 1, 2, None) != OK                    # null arrays


def test_constructor_defaults_and_validation():
    from myrtle_vision.utils.random_erasing import RandomErasing
    e = RandomErasing()
    assert (e.probability, e.mode, e.min_area, e.max_area, e.min_count, e.max_count) == (0.25, "pixel", 0.02, 1 / 3, 1, 1)
    assert e.log_ratio == (math.log(0.3), math.log(1 / 0.3)) and e.thr == 1 << 30
    assert e.state is None and e.last_boxes is None
    assert RandomErasing(probability=1.0).thr == 1 << 32 and RandomErasing(probability=0.0).thr == 0
    assert RandomErasing(min_count=2).max_count == 2 and RandomErasing(min_count=2, max_count=5).max_count == 5
    assert RandomErasing(min_aspect=0.5, max_aspect=4.0).log_ratio == (math.log(0.5), math.log(4.0))
    bad = [dict(probability=-0.1), dict(probability=1.5), dict(probability=float("nan")), dict(mode="noise"), dict(min_area=0.0),
           dict(min_area=0.5, max_area=0.4), dict(max_area=1.5), dict(min_aspect=0.0), dict(min_aspect=-1.0), dict(max_aspect=0.0),
           dict(min_count=0), dict(min_count=3, max_count=2), dict(max_count=9), dict(min_count=9), dict(min_count=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            RandomErasing(**kw)


def test_the_new_config_differs_in_the_three_keys_only():
    base = json.load(open(os.path.join(CFG_DIR, "vit_base_mixup.json")))
    re_ = json.load(open(os.path.join(CFG_DIR, "vit_base_mixup_re.json")))
    assert (re_["train_config"].pop("reprob"), re_["train_config"].pop("remode"), re_["train_config"].pop("recount")) == (0.25, "pixel", 1)
    assert re_ == base


def test_engine_builds_the_eraser_from_the_keys():
    from myrtle_vision import engine
    cfg = json.load(open(os.path.join(CFG_DIR, "vit_base_mixup_re.json")))["train_config"]
    e = engine._random_eraser("classification", cfg)
    assert (e.probability, e.mode, e.min_count, e.max_count) == (0.25, "pixel", 1, 1)
    e = engine._random_eraser("classification", {"reprob": 0.5, "remode": "rand", "recount": 3})
    assert (e.probability, e.mode, e.min_count, e.max_count) == (0.5, "rand", 3, 3)
    with pytest.raises(ValueError):
        engine._random_eraser("classification", {"reprob": 0.5, "remode": "noise"})


@pytest.mark.parametrize("key,value", [("reprob", 0.25), ("remode", "pixel"), ("recount", 1)])
@pytest.mark.parametrize("task", ["segmentation", "detection"])
def test_engine_refuses_the_keys_on_another_task(task, key, value):
    from myrtle_vision import engine
    with pytest.raises(ValueError, match=key):
        engine._random_eraser(task, {key: value})


@pytest.mark.parametrize("task,folder,name", [("segmentation", "segmentation", "seg_tiny.json"), ("detection", "detection", "yolos_tiny.json")])
def test_train_worker_refuses_reprob_before_any_work(tmp_path, task, folder, name):
    """Through ``train_worker`` itself: the error comes before the device is looked for, so this runs anywhere."""
    from myrtle_vision.engine import train_worker
    cfg = json.load(open(os.path.join(ROOT, folder, "train_configs", name)))
    data = json.load(open(os.path.join(ROOT, folder, "data_configs", "data_config.json")))
    cfg["data_config_path"] = str(tmp_path / "data_config.json")
    json.dump(data, open(cfg["data_config_path"], "w"))
    cfg["train_config"]["reprob"] = 0.25
    with pytest.raises(ValueError, match="reprob"):
        train_worker(0, 1, cfg, task)


def test_a_config_without_the_keys_does_not_import_the_eraser(monkeypatch):
    from myrtle_vision import engine
    monkeypatch.delitem(sys.modules, "myrtle_vision.utils.random_erasing", raising=False)
    for name in ("vit_base_mixup.json", "vit_tiny.json", "deit_tiny.json"):
        cfg = json.load(open(os.path.join(CFG_DIR, name)))["train_config"]
        assert engine._random_eraser("classification", cfg) is None
    assert engine._random_eraser("classification", {"reprob": 0.0, "remode": "rand", "recount": 2}) is None
    assert engine._random_eraser("segmentation", {}) is None and engine._random_eraser("detection", {}) is None
    assert "myrtle_vision.utils.random_erasing" not in sys.modules


# ---------------------------------------------------------------- the restatement's statistics at a fixed (seed, step)
def test_erased_share_boxes_and_counts():
    n, p, H, W = 4096, 0.25, 224, 224
    boxes, attempts, _ = R.draw(n, H, W, SEED, STEP, probability=p)
    erased = (boxes[:, 0, 2:] > 0).any(axis=1)          # at 224^2 and the default areas no accepted box has zero extent
    print(f"erased {int(erased.sum())} of {n}: {(erased.sum() - n * p) / math.sqrt(n * p * (1 - p)):+.2f} sigma")
    assert abs(int(erased.sum()) - n * p) <= 4.0 * math.sqrt(n * p * (1 - p))
    top, left, h, w = (boxes[..., i] for i in range(4))
    assert (h < H).all() and (w < W).all() and (top >= 0).all() and (left >= 0).all()
    assert (top + h <= H).all() and (left + w <= W).all()
    assert (boxes[~erased] == 0).all()
    # the erased area is uniform over [min_area, max_area] of the image up to the rounding of h and w
    share = (h * w)[erased, 0] / (H * W)
    assert 0.015 < share.min() and share.max() < 0.35 and abs(share.mean() - (0.02 + 1 / 3) / 2) < 0.01
    # count covers its range; slots beyond the count stay empty
    boxes, _, _ = R.draw(512, 64, 64, SEED, STEP, probability=1.0, min_count=2, max_count=5)
    counts = ((boxes[..., 2] > 0) & (boxes[..., 3] > 0)).sum(axis=1)
    assert set(counts.tolist()) == {2, 3, 4, 5}
    assert all(np.array_equal(np.nonzero(row)[0], np.arange(c)) for row, c in zip(((boxes[..., 2] > 0) & (boxes[..., 3] > 0)), counts))
    # probability 1 erases every sample, probability 0 none
    assert (R.draw(300, 64, 64, SEED, STEP, probability=1.0)[0][:, 0, 2] > 0).all()
    assert not R.draw(300, 64, 64, SEED, STEP, probability=0.0)[0].any()


def test_step_and_seed_move_the_boxes():
    a = R.draw(256, 224, 224, SEED, STEP)[0]
    assert np.array_equal(a, R.draw(256, 224, 224, SEED, STEP)[0])
    assert not np.array_equal(a, R.draw(256, 224, 224, SEED, STEP + 1)[0])
    assert not np.array_equal(a, R.draw(256, 224, 224, SEED + 1, STEP)[0])


def test_the_three_streams_share_no_counter():
    B, Ch, H, W = 64, 3, 32, 48
    _, _, calls = R.draw(B, H, W, SEED, STEP, probability=1.0, min_count=1, max_count=8, min_area=0.9, max_area=0.9, min_aspect=0.1)
    draw_c = R.counters(R.TAG_DRAW, calls, STEP)
    every_draw = R.counters(R.TAG_DRAW, [b * R.SAMPLE_STRIDE + j for b in range(B) for j in range(1 + R.MAX_COUNT * R.ATTEMPTS)], STEP)
    colour_c = R.counters(R.TAG_COLOUR, [(b * R.MAX_COUNT + k) * Ch + c for b in range(B) for k in range(R.MAX_COUNT) for c in range(Ch)], STEP)
    pixel_c = R.counters(R.TAG_PIXEL, np.arange(B * Ch * H * W, dtype=np.uint64) >> np.uint64(2), STEP)
    assert draw_c <= every_draw and len(calls) == len(draw_c) > B                      # no call index is used twice
    assert len(every_draw) == B * 81 and len(colour_c) == B * 8 * Ch and len(pixel_c) == B * Ch * H * W // 4
    assert not (every_draw & colour_c) and not (every_draw & pixel_c) and not (colour_c & pixel_c)
    # ... nor with the next step's, and an index beyond 2^32 keeps its tag
    assert not (every_draw | colour_c | pixel_c) & R.counters(R.TAG_PIXEL, np.arange(4096, dtype=np.uint64), STEP + 1)
    assert R.counters(R.TAG_PIXEL, [(1 << 55) + 5], 7) == {(5, (3 << 24) | (1 << 23), 7, 0)}


def test_pixel_normals_are_standard_normal():
    n = 1 << 17
    z = R.pixel_normals(np.arange(n, dtype=np.uint64), SEED, STEP)
    mean, var = float(z.mean()), float(z.var())
    print(f"n = {n}: mean {mean:+.5f} (bar {4 / math.sqrt(n):.5f}), variance {var:.5f} (bar 1 +- {4 * math.sqrt(2 / n):.5f})")
    assert np.isfinite(z).all()
    assert abs(mean) <= 4.0 / math.sqrt(n) and abs(var - 1.0) <= 4.0 * math.sqrt(2.0 / n)
    # cos and sin branches of one pair are uncorrelated, and the step moves the stream
    assert abs(float(np.mean(z[0::2] * z[1::2]))) <= 4.0 / math.sqrt(n / 2)
    assert not np.array_equal(z[:64], R.pixel_normals(np.arange(64, dtype=np.uint64), SEED, STEP + 1))


def test_fill_restatement_last_box_wins():
    boxes = np.array([[[0, 0, 3, 3], [2, 2, 3, 3], [0, 0, 0, 0]]], dtype=np.int32)
    owner = R.winners(boxes, 6, 6)[0]
    assert owner[0, 0] == 0 and owner[2, 2] == 1 and owner[4, 4] == 1 and owner[5, 5] == -1 and (owner >= 0).sum() == 9 + 9 - 1
    own, val = R.fill64((1, 2, 6, 6), boxes, "rand", SEED, STEP)
    assert len({float(v) for v in val[0, 0][own[0] == 1]}) == 1 and val[0, 0, 2, 2] != val[0, 0, 0, 0] and val[0, 0, 0, 0] != val[0, 1, 0, 0]
    assert np.array_equal(R.bf16_round(np.array([1.0, 1.00390625, 1.01171875, -1.00390625], dtype=np.float32)),
                          np.array([1.0, 1.0, 1.015625, -1.0], dtype=np.float32))
