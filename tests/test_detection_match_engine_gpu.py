"""GPU: the detection loop with ``train_config["device_matcher"]``.  The device solver returns scipy's assignment, so a run with
it and a run without it, from the same seed on the same synthetic directory, are the same run: every per-step loss and the epoch
record (training loss, validation loss, AP) are equal bit for bit.  And the loop's read of the loss brings the solver's status along and raises
scipy's message for an image that was not solved."""
import copy
import glob
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _config(tmp_path, device_matcher):
    from conftest import ROOT
    from myrtle_vision.datasets.synthetic import make_dior_coco
    cfg = json.load(open(os.path.join(ROOT, "detection", "train_configs", "yolos_tiny.json")))
    data = json.load(open(os.path.join(ROOT, "detection", "data_configs", "data_config.json")))
    data["dataset_path"] = make_dior_coco(str(tmp_path / "DIOR-COCO"), counts=(8, 4, 4))
    data.update(train_subset=None, valid_subset=None)
    ratio, norm = {"max_size_ratio": [4, 3]}, {"Normalize": {"Mean": [0.5] * 3, "Std": [0.5] * 3}}
    data["transform_ops_train"] = {"RandomHorizontalFlip": None, "RandomSelect": {
        "RandomResize": {"scales": [64, 80, 96], **ratio},
        "Compose": {"PreRandomResize": {"scales": [96, 112]}, "RandomSizeCrop": [64, 96], "PostRandomResize": {"scales": [64, 80], **ratio}}},
        **norm}
    data["transform_ops_val"] = {"RandomResize": {"scales": [96], **ratio}, **norm}
    dpath = str(tmp_path / "data_config.json")
    json.dump(data, open(dpath, "w"))
    cfg["data_config_path"] = dpath
    cfg["train_config"].update(output_directory=str(tmp_path / "ckpt"), epochs=1, local_batch_size=2, global_batch_size=2,
                               distributed=False, pretrained_backbone=None, device_matcher=device_matcher)
    cfg["vit_config"].update(embed_dim=64, depth=2, heads=1, mlp_dim=128, num_det_tokens=10, precision="fp32")
    return cfg


def test_device_matcher_trains_the_same_run_as_the_host_matcher(tmp_path, monkeypatch):
    from myrtle_vision import engine
    from myrtle_vision.models.matcher import HungarianMatcher
    built = []
    init = HungarianMatcher.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        built.append(self.assignment)
    monkeypatch.setattr(HungarianMatcher, "__init__", spy)
    rows = {}
    for device_matcher in (False, True):
        sub = tmp_path / ("device" if device_matcher else "host")
        sub.mkdir()
        engine.launch_training(copy.deepcopy(_config(sub, device_matcher)), "detection")
        (out,) = glob.glob(str(sub / "ckpt_*"))
        rows[device_matcher] = [json.loads(line) for line in open(os.path.join(out, "train_log.jsonl"))]
    assert built == ["host", "device"]                                      # the loop built the matcher the config asked for
    assert [r["iteration"] for r in rows[True] if "iteration" in r] == [1, 2, 3, 4]
    assert rows[True] == rows[False]                                        # per-step losses, epoch loss, val_loss, ap, lr


class _Criterion:
    def __init__(self, status):
        self.match_status = status


def test_the_loss_read_checks_the_solver_status():
    from myrtle_vision.engine import _loss_to_host
    loss = torch.tensor(1.2345678, device="cuda")
    want = float(loss)
    assert _loss_to_host(loss, _Criterion(None)) == want                    # host mode: no status
    assert _loss_to_host(loss, _Criterion(torch.zeros(3, dtype=torch.int32, device="cuda"))) == want
    with pytest.raises(ValueError, match="^matrix contains invalid numeric entries$"):
        _loss_to_host(loss, _Criterion(torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError, match="^cost matrix is infeasible$"):
        _loss_to_host(loss, _Criterion(torch.tensor([0, 0, 2], dtype=torch.int32, device="cuda")))
