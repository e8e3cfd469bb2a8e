"""Host-side checks of the YOLOS detection feature: fixtures, the generator's torchvision stand-in, module interfaces."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

import detection_ref as ref

CASES = ["micro_det", "base_det"]


def _generator_module():
    spec = importlib.util.spec_from_file_location("gen_golden_detection", os.path.join(GOLDEN, "gen_golden_detection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # top level imports numpy / torch / scipy only; the reference is imported in run_case
    return mod


@pytest.mark.parametrize("name", CASES)
def test_fixture_holds_every_recorded_output(name):
    arrays, meta = load_golden(name)
    B, Q, C1 = meta["batch"], meta["num_queries"], meta["kwargs"]["num_classes"] + 1
    assert arrays["pred_logits"].shape == (B, Q, C1) and arrays["pred_boxes"].shape == (B, Q, 4)
    for k in ("loss_ce", "class_error", "cardinality_error", "loss_bbox", "loss_giou", "total"):
        assert arrays[k].shape == () and np.isfinite(arrays[k])
    sizes = meta["targets"]["sizes"]
    assert len(sizes) == B and 0 in sizes and max(sizes) <= 12
    for b, n in enumerate(sizes):
        assert arrays[f"index_i:{b}"].shape == arrays[f"index_j:{b}"].shape == (min(n, Q),)
        assert arrays[f"index_i:{b}"].dtype == np.int64
        assert arrays[f"tgt_labels:{b}"].shape == (n,) and arrays[f"tgt_boxes:{b}"].shape == (n, 4)
        assert (arrays[f"tgt_boxes:{b}"][:, 2:] > 0.02).all()
    for k in ("decoder.class_embed.weight", "decoder.class_embed.bias", "decoder.bbox_embed.weight", "decoder.bbox_embed.bias"):
        assert arrays[f"grad:{k}"].shape == tuple(meta["param_shapes"][k]) and f"gsum:{k}" in arrays
    assert set(meta["unused_params"]) == {"pos_embedding_det", "det_tokens"}          # the reference never concatenates them
    assert all(f"gsum:{k}" in arrays for k in meta["param_shapes"] if k not in meta["unused_params"])
    tie = meta["tie_check"]
    assert tie["stable"] and tie["draws"] == 32 and tie["eps"] == 1e-4 and tie["min_margin"] > 2 * 12 * tie["eps"]
    total = sum(float(arrays[k]) * w for k, w in meta["weight_dict"].items())
    assert abs(total - float(arrays["total"])) < 1e-5 * abs(total)


@pytest.mark.parametrize("name", CASES)
def test_fixture_targets_follow_the_recorded_formula(name):
    gen = _generator_module()
    arrays, meta = load_golden(name)
    targets = gen.det_targets(name, meta["targets"]["seed"], meta["batch"], meta["kwargs"]["num_classes"])
    for b, t in enumerate(targets):
        assert np.array_equal(t["labels"].numpy(), arrays[f"tgt_labels:{b}"])
        assert np.array_equal(t["boxes"].numpy(), arrays[f"tgt_boxes:{b}"])


@pytest.mark.parametrize("name", CASES)
def test_fixture_matched_boxes_keep_clear_of_the_box_losses_kinks(name):
    """Recomputed from the stored arrays: no matched pair within the generator's margins of a point where L1's sign or a GIoU
    max / min / clamp selection changes (there a gradient comparison would judge rounding direction, not accuracy)."""
    gen = _generator_module()
    arrays, meta = load_golden(name)
    kc = meta["kink_check"]
    assert kc["margin"] == gen.KINK_MARGIN == 1.5e-2 and kc["corner_factor"] == 1.5
    gaps = [gen.kink_gap(arrays["pred_boxes"][b][arrays[f"index_i:{b}"]], arrays[f"tgt_boxes:{b}"][arrays[f"index_j:{b}"]])
            for b in range(meta["batch"])]
    assert min(gaps) >= 1.0 and min(gaps) == pytest.approx(kc["min_gap_in_margins"], rel=1e-5)
    assert gen.kink_gap(np.array([[0.5, 0.5, 0.2, 0.2]]), np.array([[0.5 + 1e-3, 0.4, 0.3, 0.3]])) < 1.0      # a coordinate on a kink
    assert gen.kink_gap(np.array([[0.5, 0.5, 0.2, 0.2]]), np.array([[0.7, 0.7, 0.2, 0.2]])) < 1.0            # touching boxes


@pytest.mark.parametrize("name", CASES)
def test_torchvision_standin_giou_equals_direct_fp64_evaluation(name):
    """The generator's ``generalized_box_iou`` / ``box_convert`` on the fixture's boxes against the formula written out per pair
    in Python floats (fp64): intersection over union minus the share of the enclosing box that the union leaves empty."""
    gen = _generator_module()
    arrays, meta = load_golden(name)
    for b, n in enumerate(meta["targets"]["sizes"]):
        if n == 0:
            continue
        pred, tgt = arrays["pred_boxes"][b].astype(np.float64), arrays[f"tgt_boxes:{b}"].astype(np.float64)
        got = gen.generalized_box_iou(gen.box_convert(torch.from_numpy(pred), "cxcywh", "xyxy"),
                                      gen.box_convert(torch.from_numpy(tgt), "cxcywh", "xyxy")).numpy()
        assert got.shape == (len(pred), n)
        for q in range(0, len(pred), 7):
            for t in range(n):
                ax0, ay0, ax1, ay1 = pred[q, 0] - 0.5 * pred[q, 2], pred[q, 1] - 0.5 * pred[q, 3], pred[q, 0] + 0.5 * pred[q, 2], pred[q, 1] + 0.5 * pred[q, 3]
                bx0, by0, bx1, by1 = tgt[t, 0] - 0.5 * tgt[t, 2], tgt[t, 1] - 0.5 * tgt[t, 3], tgt[t, 0] + 0.5 * tgt[t, 2], tgt[t, 1] + 0.5 * tgt[t, 3]
                inter = max(min(ax1, bx1) - max(ax0, bx0), 0.0) * max(min(ay1, by1) - max(ay0, by0), 0.0)
                union = (ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0) - inter
                hull = max(max(ax1, bx1) - min(ax0, bx0), 0.0) * max(max(ay1, by1) - min(ay0, by0), 0.0)
                want = inter / union - (hull - union) / hull
                assert abs(got[q, t] - want) < 1e-12, (b, q, t)
        # the test-side restatement is the same function
        mine = ref.giou(ref.xyxy(torch.from_numpy(pred))[:, None, :], ref.xyxy(torch.from_numpy(tgt))[None, :, :]).numpy()
        assert np.abs(mine - got).max() < 1e-12


@pytest.mark.parametrize("name", CASES)
def test_state_dict_and_unused_parameters(name):
    from myrtle_vision.models.vit import ViT
    _, meta = load_golden(name)
    vit = ViT(patch_size=16, q_format="FP32", **meta["kwargs"])
    assert list(vit.state_dict().keys()) == meta["state_keys"]
    assert set(vit.unused_parameter_names()) == set(meta["unused_params"])
    live = ViT(patch_size=16, q_format="FP32", live_det_tokens=True, **meta["kwargs"])
    assert live.unused_parameter_names() == () and list(live.state_dict().keys()) == meta["state_keys"]


def test_live_det_tokens_is_for_the_detection_decoder_only():
    from myrtle_vision.models.vit import ViT
    with pytest.raises(ValueError, match="live_det_tokens"):
        ViT(decoder="classification", image_size=224, patch_size=16, num_classes=5, dim=64, depth=1, heads=1, mlp_dim=64,
            live_det_tokens=True)


def test_module_classes_import_with_the_reference_interfaces():
    from myrtle_vision.models.detector import PostProcess, SetCriterion
    from myrtle_vision.models.matcher import HungarianMatcher
    m = HungarianMatcher()
    assert (m.cost_class, m.cost_bbox, m.cost_giou) == (1, 1, 1)
    with pytest.raises(AssertionError, match="all costs cant be 0"):
        HungarianMatcher(cost_class=0, cost_bbox=0, cost_giou=0)
    wd = {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0}
    crit = SetCriterion(20, matcher=m, weight_dict=wd, eos_coef=0.1, losses=["labels", "boxes", "cardinality"])
    assert list(crit.state_dict().keys()) == ["empty_weight"]
    w = crit.empty_weight
    assert w.shape == (21,) and w.dtype == torch.float32 and bool((w[:-1] == 1).all()) and float(w[-1]) == pytest.approx(0.1)
    assert crit.num_classes == 20 and crit.matcher is m and crit.weight_dict is wd and crit.eos_coef == 0.1
    assert isinstance(PostProcess(), torch.nn.Module)
    bad = SetCriterion(20, matcher=m, weight_dict=wd, eos_coef=0.1, losses=["masks"])
    with pytest.raises(AssertionError, match="do you really want to compute masks loss"):
        bad({"pred_logits": torch.zeros(1, 2, 21), "pred_boxes": torch.zeros(1, 2, 4)}, [{"labels": torch.zeros(0, dtype=torch.long), "boxes": torch.zeros(0, 4)}])


def test_detection_has_no_cpu_path():
    from myrtle_vision.models.detector import PostProcess, SetCriterion
    from myrtle_vision.models.matcher import HungarianMatcher
    from myrtle_vision.models.vit import DetectionDecoder
    out = {"pred_logits": torch.zeros(1, 2, 21), "pred_boxes": torch.full((1, 2, 4), 0.5)}
    tgt = [{"labels": torch.zeros(1, dtype=torch.long), "boxes": torch.full((1, 4), 0.5)}]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DetectionDecoder(64, 20, 2)(torch.zeros(1, 5, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HungarianMatcher()(out, tgt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SetCriterion(20, HungarianMatcher(), {}, 0.1, ["labels"])(out, tgt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PostProcess()(out, torch.tensor([[480, 640]]))


def test_parity_table_covers_every_quantity_with_the_factor_of_eight():
    table = ref.read_parity_table(os.path.join(ROOT, "profiles", "detection_parity.txt"))
    assert set(table) == set(ref.QUANTITIES)
    for q, (base, bound) in table.items():
        assert bound == pytest.approx(ref.PARITY_FACTOR * base, rel=1e-5), q
        assert base < 1e-5, q                                     # an fp32 evaluation of O(1) formulas


def test_reference_matching_is_one_to_one_and_covers_min_of_queries_and_targets():
    for case in ref.KERNEL_CASES:
        B, Q, C, sizes = case
        logits, boxes, targets, _, _ = ref.case_inputs(case)
        for (i, j), n in zip(ref.match(logits, boxes, targets), sizes):
            assert len(i) == len(j) == min(Q, n) and len(set(i)) == len(i) and len(set(j)) == len(j)
