"""Record what the reference's detection transforms produce for the samples of tests/detection_data_samples.py.

    python tests/golden/gen_golden_detection_data.py /path/to/reference/src/myrtle_vision/transforms/detection.py

-> tests/golden/detection_transforms_ref.json: per (chain, sample, seed) the output size, the kept labels, the normalised
boxes and the areas (fp32 values written as the doubles they equal, so JSON returns them exactly).  The chains are the two
``transform_ops_*`` sections of the reference's detection data config, kept as tests/golden/detection_transform_ops_ref.json.

The reference module imports torchvision, which is not needed for what it computes on PIL images: the few functions it calls
are supplied here as an in-memory stand-in written from torchvision's documented behaviour (crop / hflip / resize on PIL images
are ``Image.crop`` / ``Image.transpose`` / ``Image.resize(BILINEAR)``; ``RandomCrop.get_params`` draws top then left with
``torch.randint`` and draws nothing for a full-size crop; ``box_convert`` xyxy -> cxcywh).  The fixture therefore pins the
reference's own code -- size rule, draw order, box / area arithmetic, config parsing -- given that stand-in.
"""
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from detection_data_samples import cases, data_config, make_sample  # noqa: E402


def _standin():
    tv, tr, fn, ops, boxes = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms",
                                                            "torchvision.transforms.functional", "torchvision.ops",
                                                            "torchvision.ops.boxes"))
    tv._is_tracing = lambda: False

    class RandomCrop:
        @staticmethod
        def get_params(img, output_size):
            w, h = img.size
            th, tw = output_size
            if h < th or w < tw:
                raise ValueError("crop larger than the image")
            if w == tw and h == th:
                return 0, 0, h, w
            i = torch.randint(0, h - th + 1, size=(1,)).item()
            j = torch.randint(0, w - tw + 1, size=(1,)).item()
            return i, j, th, tw

    tr.RandomCrop, tr.RandomErasing = RandomCrop, object
    fn.crop = lambda img, top, left, height, width: img.crop((left, top, left + width, top + height))
    fn.hflip = lambda img: img.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    fn.resize = lambda img, size: img.resize(tuple(int(s) for s in size[::-1]), Image.Resampling.BILINEAR)
    fn.to_tensor = lambda img: torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255)
    fn.normalize = lambda t, mean, std: (t - torch.tensor(mean).view(-1, 1, 1)) / torch.tensor(std).view(-1, 1, 1)

    def box_convert(b, in_fmt, out_fmt):
        assert (in_fmt, out_fmt) == ("xyxy", "cxcywh")
        x0, y0, x1, y1 = b.unbind(-1)
        return torch.stack(((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0), dim=-1)

    boxes.box_convert = box_convert
    tv.transforms, tv.ops, tr.functional, ops.boxes = tr, ops, fn, boxes
    for m in (tv, tr, fn, ops, boxes):
        sys.modules[m.__name__] = m


def main(path):
    _standin()
    spec = importlib.util.spec_from_file_location("reference_detection_transforms", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    cfg, rows = data_config(), []
    for chain, name, seed in cases():
        img, target = make_sample(name)
        random.seed(seed)
        torch.manual_seed(seed)
        out, t = ref.from_config(cfg[chain])(img, target)
        rows.append({"chain": chain, "sample": name, "seed": seed, "shape": list(out.shape), "size": t["size"].tolist(),
                     "labels": t["labels"].tolist(), "boxes": t["boxes"].double().tolist(), "area": t["area"].double().tolist(),
                     "pixel_sum": float(out.double().sum())})
    with open(os.path.join(HERE, "detection_transforms_ref.json"), "w") as f:
        json.dump(rows, f, indent=0)
    print(f"{len(rows)} cases")


if __name__ == "__main__":
    main(sys.argv[1])
