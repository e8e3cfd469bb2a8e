"""Stochastic depth (drop path), host side: the C ABI of the three entry points, the per-block rates, the state-dict format, the
config key, the threshold / scale tables and the numpy restatement of the draw (tests/drop_path_ref.py).  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from drop_path_ref import draw_table, keep_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(decoder="classification", image_size=80, patch_size=16, num_classes=5, dim=128, depth=3, heads=2, mlp_dim=256)


def test_entry_points_are_declared_bound_and_built():
    from myrtle_vision.hip import build, lib
    assert lib.SIGNATURES["mv_drop_path_draw"] == ("pppp" "ii" "p", ctypes.c_int)
    assert lib.SIGNATURES["mv_drop_path_add"] == ("ppp" "il" "p", ctypes.c_int)
    assert lib.SIGNATURES["mv_row_scale"] == ("pipip" "il" "p", ctypes.c_int)
    assert "drop_path.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "myrtle_vision_hip.h")).read()
    for name in ("mv_drop_path_draw", "mv_drop_path_add", "mv_row_scale"):
        assert f"int {name}(" in header
    handle = lib.lib()
    # argument checks answered on the host, before any launch: nothing to do is MV_OK, a dtype outside fp32 / bf16 is refused
    assert handle.mv_drop_path_draw(None, None, None, None, 0, 7, None) == 0
    assert handle.mv_drop_path_add(None, None, None, 0, 12, None) == 0
    assert handle.mv_row_scale(None, lib.MV_F32, None, lib.MV_BF16, None, 3, 0, None) == 0
    unsupported = -4
    assert handle.mv_row_scale(1 << 20, lib.MV_I8, 1 << 20, lib.MV_F32, 1 << 20, 3, 4, None) == unsupported
    assert handle.mv_row_scale(1 << 20, lib.MV_F32, 1 << 20, lib.MV_F16, 1 << 20, 3, 4, None) == unsupported
    assert handle.mv_row_scale(1 << 20, 7, 1 << 20, 7, 1 << 20, 3, 4, None) == unsupported
    assert handle.mv_drop_path_draw(None, None, None, None, 1 << 13, 1 << 12, None) != 0          # R * B > 2^24


def test_philox_has_one_definition_shared_with_dropout():
    csrc = os.path.join(ROOT, "myrtle-vision_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f))
            and "void philox4x32_10(" in open(os.path.join(csrc, f)).read()]
    assert defs == ["philox.h"]
    for f in ("elementwise.hip", "drop_path.hip"):
        assert '#include "philox.h"' in open(os.path.join(csrc, f)).read()


@pytest.mark.parametrize("depth", [1, 2, 3, 12])
def test_block_rates_are_linspace(depth):
    from myrtle_vision.models.vit import Transformer, drop_path_rates
    rates = drop_path_rates(0.3, depth)
    assert np.allclose(rates, torch.linspace(0, 0.3, depth).tolist() if depth > 1 else [0.0], atol=1e-7)
    tr = Transformer(64, depth, 1, 64, 128, 0.0, False, drop_path_rate=0.3)
    assert tr.block_drop_rates == rates
    live = [i for i, p in enumerate(rates) if p > 0]
    assert list(tr.drop_path_rows) == [(i, j) for i in live for j in (0, 1)]              # both branches of a block, in order
    assert list(tr.drop_path_rows.values()) == list(range(2 * len(live)))
    assert tr.drop_path.rates == [rates[i] for i in live for _ in (0, 1)]


@pytest.mark.parametrize("rate", [-0.1, 1.0, 1.5, float("nan")])
def test_bad_rates_raise(rate):
    from myrtle_vision.models.vit import ViT
    with pytest.raises(ValueError):
        ViT(drop_path_rate=rate, **KW)


def test_state_dict_format_and_initialisation_do_not_change():
    from myrtle_vision.models.vit import ViT
    torch.manual_seed(5)
    a = ViT(**KW)
    torch.manual_seed(5)
    b = ViT(drop_path_rate=0.3, **KW)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)                    # building the model draws nothing from the generator
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    assert a.transformer.drop_path.rates == [] and a.transformer.drop_path_rows == {}
    assert b.transformer.drop_path.state is None                         # device arrays: created by the first training forward


def test_get_models_reads_the_key_and_the_new_config_differs_in_it_only():
    from myrtle_vision.utils.models import get_models
    cfg_dir = os.path.join(ROOT, "classification", "train_configs")
    base = json.load(open(os.path.join(cfg_dir, "vit_base_finetune.json")))
    dp = json.load(open(os.path.join(cfg_dir, "vit_base_finetune_dp.json")))
    assert dp["vit_config"].pop("drop_path_rate") == 0.1
    assert dp == base
    small = dict(decoder="classification", image_size=80, patch_size=16, embed_dim=128, depth=3, heads=2, mlp_dim=256, dropout=0.0,
                 emb_dropout=0.0, q_format="FP32")
    config = {"vit_config": small, "data_config_path": os.path.join(ROOT, "classification", "data_configs", "data_config.json")}
    vit, _ = get_models(config)
    assert vit.transformer.block_drop_rates == [0.0, 0.0, 0.0]
    config["vit_config"] = dict(small, drop_path_rate=0.2)
    vit, _ = get_models(config)
    assert np.allclose(vit.transformer.block_drop_rates, [0.0, 0.1, 0.2])


def test_threshold_and_scale_tables():
    from myrtle_vision.hip import ops
    rates = [0.1, 0.5, 0.9, 0.25, 1.0 / 3.0, 0.0]
    thr, scale = ops.drop_path_tables(rates)
    assert thr == [int(p * 2 ** 32) for p in rates] and all(0 <= t < 2 ** 32 for t in thr)
    assert [np.float32(s) for s in scale] == [np.float32(1.0 / (1.0 - p)) for p in rates]
    assert thr[1] == 2 ** 31 and scale[1] == 2.0 and thr[5] == 0 and scale[5] == 1.0
    with pytest.raises(ValueError):
        ops.drop_path_tables([0.5, 1.0])


def test_numpy_draw_keeps_the_expected_share():
    """R * B = 4096 pairs at p = 0.25, fixed (seed, step): the keep count within 4 sigma of n (1 - p) (measured: 3062, -0.36 sigma),
    rows of the table are slices of ONE mask over R * B elements, and the step moves the stream."""
    R, B, p, seed = 16, 256, 0.25, 1234
    n = R * B
    keep = keep_rows([p] * R, B, seed, 3)
    assert abs(int(keep.sum()) - n * (1 - p)) <= 4.0 * (n * p * (1 - p)) ** 0.5
    from oracle.dropout_oracle import dropout_keep_mask, philox4x32_10
    assert np.array_equal(keep.reshape(-1), dropout_keep_mask(n, p, seed, 3))
    # the same mask from the raw Philox words and the thresholds the host hands the kernel (ops.drop_path_tables)
    from myrtle_vision.hip import ops
    thr, _ = ops.drop_path_tables([p] * R)
    i = np.arange(n // 4, dtype=np.uint64)
    words = np.stack(philox4x32_10(i, i * 0, i * 0 + 3, i * 0, seed, 0), axis=1).reshape(R, B)
    assert np.array_equal(words >= np.array(thr, dtype=np.uint64)[:, None], keep)
    table = draw_table([p] * R, B, seed, 3)
    assert table.dtype == np.float32 and set(np.unique(table).tolist()) == {0.0, float(np.float32(1.0 / 0.75))}
    assert not np.array_equal(keep, keep_rows([p] * R, B, seed, 4))
