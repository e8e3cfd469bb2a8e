"""GPU: the detection input path.  The ragged kernels (mv_image_prepare_ragged / mv_image_resize_u8_ragged) against the host
chain on the same draws, bit for bit, with guard bytes round every output; the tap limit; a micro detector on both paths; and
the detection loop end to end on the synthetic directory."""
import copy
import glob
import json
import math
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
MEAN, STD = [0.5, 0.4, 0.3], [0.5, 0.25, 0.2]
SIZES = ((37, 53), (64, 48), (80, 80), (96, 40), (40, 96))     # (height, width) of the decoded frames


def _frames():
    rng = np.random.default_rng(3)
    out = []
    for h, w in SIZES:
        b = torch.tensor([[1.0, 2.0, w / 2, h / 2], [w / 3, h / 4, w - 1.0, h - 2.0], [w - 9.0, h - 7.0, w - 0.5, h - 0.25]])
        out.append((Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
                    {"boxes": b, "labels": torch.tensor([1, 2, 3]), "image_id": torch.tensor([len(out)]),
                     "area": (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), "iscrowd": torch.zeros(3, dtype=torch.int64),
                     "orig_size": torch.tensor([h, w]), "size": torch.tensor([h, w])}))
    return out


def _carve(shape, dtype):
    """A view in the middle of a sentinel-filled allocation, itself prefilled with 0xFF bytes (NaN as fp32)."""
    n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    guard = 4096
    raw = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    raw[guard:guard + n] = 0xFF
    return raw, raw[guard:guard + n].view(dtype).view(shape), guard, n


def _device_batch(plan_samples, plan):
    """collate + apply with every output between guard bytes -> (NestedTensor, targets, intermediate | None)."""
    packed, targets = plan.collate(plan_samples)
    s_img, s_mask, s_first = plan.output_shapes(packed)
    carved = [_carve(s_img, torch.float32), _carve(s_mask, torch.bool)] + ([_carve(s_first, torch.uint8)] if s_first else [])
    nested = plan.apply(packed, "cuda", out=carved[0][1], mask=carved[1][1], stage_out=carved[2][1] if s_first else None)
    torch.cuda.synchronize()
    for raw, _, g, n in carved:
        assert bool((raw[:g] == SENTINEL).all()) and bool((raw[g + n:] == SENTINEL).all()), "a guard byte changed"
    assert nested.tensors.data_ptr() == carved[0][1].data_ptr() and nested.mask.data_ptr() == carved[1][1].data_ptr()
    assert bool(torch.isfinite(nested.tensors).all()), "an output element was left unwritten"
    assert bool((carved[1][1].view(torch.uint8) <= 1).all()), "a mask element was left unwritten"
    return nested, targets, (carved[2][1] if s_first else None)


def _both(chains, seed=0):
    """Sample i through chains[i] on the host (PIL) and on the device path (tables + kernels), from the same seeds."""
    from myrtle_vision.datasets.detection_transforms import collate_fn
    from myrtle_vision.datasets.device_transforms import DetectionDevicePlan
    frames = _frames()
    random.seed(seed)
    torch.manual_seed(seed)
    host, host_targets = collate_fn([c(img, t) for c, (img, t) in zip(chains, frames)])
    random.seed(seed)
    torch.manual_seed(seed)
    plans = [DetectionDevicePlan(chain=c) for c in chains]
    dev, dev_targets, first = _device_batch([p(img, t) for p, (img, t) in zip(plans, frames)], plans[0])
    return host, host_targets, dev, dev_targets, first


def _assert_same(host, host_targets, dev, dev_targets):
    assert dev.tensors.shape == host.tensors.shape and dev.mask.dtype == torch.bool
    assert torch.equal(dev.tensors.cpu(), host.tensors), float((dev.tensors.cpu() - host.tensors).abs().max())
    assert torch.equal(dev.mask.cpu(), host.mask)
    assert len(dev_targets) == len(host_targets)
    for a, b in zip(dev_targets, host_targets):
        assert set(a) == set(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def _chain(*ops):
    from myrtle_vision.datasets import detection_transforms as T
    return T.Compose(list(ops) + [T.ToTensor(), T.Normalize(MEAN, STD)])


class _Crop:
    def __init__(self, region):
        self.region = region

    def __call__(self, img, target):
        from myrtle_vision.datasets.detection_transforms import crop
        return crop(img, target, self.region)


def test_single_resampling_batch_is_bit_exact():
    """37x53 -> 48x64 (up, landscape, flipped); 64x48 -> 48x32 (down, portrait); 80x80 -> 112x112 = (Hmax, Wmax) (up, flipped);
    96x40 -> 96x32 (the short side already has the size: width floored, no resampling of the height); 40x96 -> 16x32 (down,
    one 16-pixel side, the smallest: zero fill on both axes)."""
    from myrtle_vision.datasets import detection_transforms as T
    flip, keep = T.RandomHorizontalFlip(p=1.0), T.RandomHorizontalFlip(p=0.0)
    chains = [_chain(flip, T.RandomResize([48])), _chain(keep, T.RandomResize([36])), _chain(flip, T.RandomResize([112])),
              _chain(keep, T.RandomResize([40])), _chain(flip, T.RandomResize([16]))]
    host, ht, dev, dt, first = _both(chains)
    assert first is None and tuple(host.tensors.shape) == (5, 3, 112, 112)
    assert [t["size"].tolist() for t in ht] == [[48, 64], [48, 32], [112, 112], [96, 32], [16, 32]]
    _assert_same(host, ht, dev, dt)
    assert float(dev.tensors[4, :, 16:, :].abs().sum()) == 0.0 and float(dev.tensors[4, :, :, 32:].abs().sum()) == 0.0
    assert not bool(dev.mask[2].any()) and int((~dev.mask[4]).sum()) == 16 * 32


def test_two_resampling_batch_is_bit_exact():
    """PreRandomResize -> crop -> PostRandomResize with the crop window at the top-left corner, at the bottom-right corner and
    strictly inside; Pillow rounds to uint8 after the first resampling, so the intermediate image is checked as well."""
    from myrtle_vision.datasets import detection_transforms as T
    flip, keep = T.RandomHorizontalFlip(p=1.0), T.RandomHorizontalFlip(p=0.0)
    chains = [_chain(flip, T.RandomResize([48]), _Crop((0, 0, 30, 40)), T.RandomResize([64])),            # 48x64: top-left corner
              _chain(keep, T.RandomResize([96]), _Crop((128 - 50, 96 - 33, 50, 33)), T.RandomResize([16])),  # 128x96: bottom-right
              _chain(flip, T.RandomResize([48]), _Crop((5, 7, 32, 36)), T.RandomResize([112])),            # 48x48: inside
              _chain(keep, T.RandomResize([64]), _Crop((9, 3, 120, 50)), T.RandomResize([32])),            # 144x64: inside, down
              _chain(keep, T.RandomResize([32]), _Crop((0, 10, 32, 40)), T.RandomResize([32]))]            # 32x64: same-size second
    host, ht, dev, dt, first = _both(chains)
    assert first is not None and [t["size"].tolist() for t in ht][0] == [64, 80]
    _assert_same(host, ht, dev, dt)
    # the uint8 intermediate = the cropped first resize, zero elsewhere
    frames = _frames()
    random.seed(0)
    for i, (c, (img, t)) in enumerate(zip(chains, frames)):
        for op in c.transforms[:3]:
            img, t = op(img, t)
        want = torch.from_numpy(np.asarray(img).copy())
        h, w = want.shape[:2]
        assert torch.equal(first[i, :h, :w].cpu(), want), i
        assert int(first[i, h:].sum()) == 0 and int(first[i, :, w:].sum()) == 0


VAL = {"RandomResize": {"scales": [48], "max_size_ratio": [3, 2]}, "Normalize": {"Mean": MEAN, "Std": STD}}
TRAIN = {"RandomHorizontalFlip": None,
         "RandomSelect": {"RandomResize": {"scales": [16, 32, 48, 64, 96], "max_size_ratio": [4, 3]},
                          "Compose": {"PreRandomResize": {"scales": [48, 64, 80]}, "RandomSizeCrop": [32, 64],
                                      "PostRandomResize": {"scales": [32, 48, 96], "max_size_ratio": [4, 3]}}},
         "Normalize": {"Mean": MEAN, "Std": STD}}


@pytest.mark.parametrize("section,seed", [(VAL, 0), (TRAIN, 1), (TRAIN, 2), (TRAIN, 5)])
def test_config_chains_are_bit_exact_on_the_same_draws(section, seed):
    """The validation chain, and the training chain (flip, then one resampling or resize-crop-resize per image, drawn per
    image: a batch mixes both) -- built by from_config from a reference-schema section."""
    from myrtle_vision.datasets.detection_transforms import from_config
    chain = from_config(section)
    host, ht, dev, dt, _ = _both([chain] * len(SIZES), seed)
    _assert_same(host, ht, dev, dt)


def test_tap_limit_raises_at_collate_and_launches_nothing(monkeypatch):
    from myrtle_vision.datasets import detection_transforms as T
    from myrtle_vision.datasets.device_transforms import MAX_TAPS, DetectionDevicePlan
    from myrtle_vision.hip import ops
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 256, (20, 1100, 3), dtype=np.uint8))
    plan = DetectionDevicePlan(chain=_chain(T.RandomResize([(16, 16)])))             # 1100 -> 16 columns: 139 taps
    sample = plan(img, _frames()[0][1])
    assert sample[0]["kh"].shape[1] > MAX_TAPS

    def launched(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(ops, "image_prepare_ragged", launched)
    monkeypatch.setattr(ops, "image_resize_u8_ragged", launched)
    with pytest.raises(ValueError, match="taps"):
        plan.collate([sample])
    monkeypatch.undo()
    # the entry point itself refuses more than 64 taps and leaves the output alone
    raw = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device="cuda")
    k = torch.zeros(1, 16, 65, dtype=torch.int32, device="cuda")
    b = torch.zeros(1, 16, 2, dtype=torch.int32, device="cuda")
    ext = torch.tensor([[16, 16]], dtype=torch.int32, device="cuda")
    out = torch.full((1, 3, 16, 16), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match="image_prepare_ragged"):
        ops.image_prepare_ragged(raw, k, b, k, b, ext, MEAN, STD, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_micro_detector_gives_identical_outputs_on_both_paths():
    """dim 64, depth 2, one head, 20 classes on a padded 3 x 48 x 80 batch (a 3 x 5 patch grid): logits and boxes from the
    device-path batch equal those from the host-path batch bit for bit; the resized position embedding of that grid is held to
    torch's bicubic F.interpolate on the CPU."""
    import torch.nn.functional as TF
    from myrtle_vision.datasets import detection_transforms as T
    from myrtle_vision.datasets.detection_transforms import collate_fn
    from myrtle_vision.datasets.device_transforms import DetectionDevicePlan
    from myrtle_vision.models.vit import ViT
    chains = [_chain(T.RandomHorizontalFlip(p=1.0), T.RandomResize([(80, 48)])), _chain(T.RandomResize([32]))]
    frames = [_frames()[2], _frames()[0]]
    host, _ = collate_fn([c(img, t) for c, (img, t) in zip(chains, frames)])
    plans = [DetectionDevicePlan(chain=c) for c in chains]
    dev, _, _ = _device_batch([p(img, t) for p, (img, t) in zip(plans, frames)], plans[0])
    assert tuple(host.tensors.shape) == (2, 3, 48, 80)
    torch.manual_seed(0)
    vit = ViT(decoder="detection", image_size=224, patch_size=16, num_classes=20, dim=64, depth=2, heads=1, mlp_dim=128,
              num_det_tokens=10, q_format="FP32", precision="fp32").cuda().eval()
    with torch.no_grad():
        a, b = vit(host.tensors.cuda()), vit(dev.tensors)
        pos = vit._pos_embedding(3, 5).cpu()
    assert a["pred_logits"].shape == (2, 10, 21) and a["pred_boxes"].shape == (2, 10, 4)
    assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])
    assert bool(torch.isfinite(a["pred_logits"]).all())
    p = vit.pos_embedding.detach().cpu()
    grid = TF.interpolate(p[0, 1:].t().reshape(1, 64, 14, 14), size=(3, 5), mode="bicubic", align_corners=False)
    want = torch.cat((p[:, :1], grid.reshape(1, 64, 15).transpose(1, 2)), dim=1)
    # fp32 dot products of 196 terms: |error| <= 196 * 2^-24 * sum|w| * max|x|, sum|w| < 2 for the 2-D bicubic kernel
    bound = 196 * 2.0 ** -24 * 2.0 * float(p.abs().max())
    assert pos.shape == want.shape and float((pos - want).abs().max()) <= bound


def _detection_config(tmp_path, device_transforms):
    from conftest import ROOT
    from myrtle_vision.datasets.synthetic import make_dior_coco
    cfg = json.load(open(os.path.join(ROOT, "detection", "train_configs", "yolos_tiny.json")))
    data = json.load(open(os.path.join(ROOT, "detection", "data_configs", "data_config.json")))
    data["dataset_path"] = make_dior_coco(str(tmp_path / "DIOR-COCO"), counts=(8, 4, 4))
    data.update(train_subset=None, valid_subset=None)
    ratio = {"max_size_ratio": [4, 3]}
    data["transform_ops_train"] = {"RandomHorizontalFlip": None, "RandomSelect": {
        "RandomResize": {"scales": [64, 80, 96], **ratio},
        "Compose": {"PreRandomResize": {"scales": [96, 112]}, "RandomSizeCrop": [64, 96], "PostRandomResize": {"scales": [64, 80], **ratio}}},
        "Normalize": {"Mean": [0.5] * 3, "Std": [0.5] * 3}}
    data["transform_ops_val"] = {"RandomResize": {"scales": [96], **ratio}, "Normalize": {"Mean": [0.5] * 3, "Std": [0.5] * 3}}
    dpath = str(tmp_path / "data_config.json")
    json.dump(data, open(dpath, "w"))
    cfg["data_config_path"] = dpath
    cfg["train_config"].update(output_directory=str(tmp_path / "ckpt"), epochs=1, local_batch_size=2, global_batch_size=2,
                               distributed=False, pretrained_backbone=None, device_transforms=device_transforms)
    cfg["vit_config"].update(embed_dim=64, depth=2, heads=1, mlp_dim=128, num_det_tokens=10, precision="fp32")
    return cfg


def test_detection_loop_end_to_end_on_both_input_paths(tmp_path, capsys):
    from myrtle_vision.engine import evaluate, launch_training
    first_loss = {}
    for device_transforms in (True, False):
        sub = tmp_path / ("device" if device_transforms else "host")
        sub.mkdir()
        cfg = _detection_config(sub, device_transforms)
        launch_training(copy.deepcopy(cfg), "detection")
        out_dirs = glob.glob(str(sub / "ckpt_*"))
        assert len(out_dirs) == 1
        rows = [json.loads(line) for line in open(os.path.join(out_dirs[0], "train_log.jsonl"))]
        steps, epochs = [r for r in rows if "iteration" in r], [r for r in rows if "epoch" in r]
        assert [r["iteration"] for r in steps] == [1, 2, 3, 4] and len(epochs) == 1          # 8 images, batches of 2
        assert all(math.isfinite(r["loss"]) for r in steps) and math.isfinite(epochs[0]["loss"])
        assert math.isfinite(epochs[0]["val_loss"]) and 0.0 <= epochs[0]["ap"] <= 1.0
        first_loss[device_transforms] = steps[0]["loss"]
        ckpt = os.path.join(out_dirs[0], "vit_epoch0")
        assert os.path.exists(ckpt)
        ck = torch.load(ckpt, map_location="cpu", weights_only=False)
        assert set(ck) == {"model", "optimizer", "lr_scheduler", "iteration"} and ck["iteration"] == 4
        cfg2 = copy.deepcopy(cfg)
        cfg2["train_config"]["checkpoint_path"] = ckpt
        res = evaluate(cfg2, "detection")
        assert len(res["stats"]) == 12 and 0.0 <= res["AP"] <= 1.0
    assert first_loss[True] == first_loss[False]
    assert "nan" not in capsys.readouterr().out.lower()
