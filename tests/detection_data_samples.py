"""Shared inputs of tests/test_detection_data_cpu.py, tests/test_detection_data_gpu.py and the fixture generator
tests/golden/gen_golden_detection_data.py: synthetic (PIL image, target) samples and the (chain, sample, seed) cases.

The samples cover: w < h, w > h, w == h; a short side already equal to the validation size (800); the max_size clamp active
(aspect ratio 2.5 at size 800: 2000 > 1333); boxes that a crop cuts or removes (small boxes in every corner, one spanning
box); an image without boxes."""
import json
import os

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (width, height, boxes xyxy in pixels)
_CORNERS = lambda w, h: [[2, 3, 30, 28], [w - 33, 4, w - 3, 30], [5, h - 31, 36, h - 2], [w - 40, h - 35, w - 1, h - 1],
                         [w * 0.25, h * 0.25, w * 0.75, h * 0.8], [w * 0.5 - 7.5, h * 0.5 - 6.25, w * 0.5 + 9.75, h * 0.5 + 11.5]]
SAMPLES = {
    "wide": (500, 400, _CORNERS(500, 400)),
    "tall": (400, 500, _CORNERS(400, 500)),
    "square": (480, 480, _CORNERS(480, 480)),
    "short_is_800": (1000, 800, _CORNERS(1000, 800)),
    "clamped": (1000, 400, _CORNERS(1000, 400)),
    "no_boxes": (450, 410, []),
}
SEEDS = (0, 1, 2, 3, 4, 5)


def data_config():
    """The reference's own ``transform_ops_train`` / ``transform_ops_val`` sections, unmodified (a fixture: the shipped
    detection/data_configs/data_config.json is this project's and may change without moving the recorded outputs)."""
    with open(os.path.join(ROOT, "tests", "golden", "detection_transform_ops_ref.json")) as f:
        return json.load(f)                                    # key order = chain order


def make_sample(name):
    w, h, boxes = SAMPLES[name]
    rng = np.random.default_rng(sorted(SAMPLES).index(name))
    img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    boxes = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    n = len(boxes)
    target = {"boxes": boxes, "labels": torch.arange(n, dtype=torch.int64) % 20, "image_id": torch.tensor([7]),
              "area": ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])), "iscrowd": torch.zeros(n, dtype=torch.int64),
              "orig_size": torch.as_tensor([h, w]), "size": torch.as_tensor([h, w])}
    return img, target


def cases():
    """(chain, sample name, seed): every sample through both chains under every seed (the validation chain draws nothing)."""
    out = [("transform_ops_val", name, 0) for name in SAMPLES]
    out += [("transform_ops_train", name, seed) for name in SAMPLES for seed in SEEDS]
    return out
