"""COCO-format detection dataset read with ``json`` alone (reference: ``src/myrtle_vision/datasets/coco.py`` on top of
torchvision's ``CocoDetection`` and pycocotools).

``CocoDetection(img_folder, ann_file, transforms)[i]`` -> (image, target) with the reference's target dict: ``boxes`` fp32
[T, 4] xyxy in pixels (COCO's xywh converted, clamped to the frame, empty boxes dropped), ``labels`` int64 [T], ``image_id``
int64 [1], ``area`` / ``iscrowd`` [T] (crowd annotations are removed before anything else), ``orig_size`` / ``size`` int64
[2] = (h, w).  Images are indexed in ascending image-id order, as pycocotools' ``sorted(imgs.keys())``.

``dataset.coco`` is a ``CocoGroundTruth``: the unfiltered annotations per image id, which is what the evaluator scores against
(crowd boxes included: COCO's protocol treats them as ignore regions).  ``coco_from_dataset`` finds it through a ``Subset``.
With a ``device_plan`` (``device_transforms.DetectionDevicePlan``) the sample is (packed frame + tables, target) instead.
"""
import json
import os

import torch
import torch.utils.data
from PIL import Image


class CocoGroundTruth:
    """The parts of a COCO annotation file the dataset and the evaluator read: ``imgs`` id -> image record, ``cats`` id ->
    category record, ``img_to_anns`` id -> list of annotation records (file order)."""

    def __init__(self, annotation_file=None, dataset=None):
        if dataset is None:
            with open(annotation_file) as f:
                dataset = json.load(f)
        self.dataset = dataset
        self.imgs = {im["id"]: im for im in dataset.get("images", [])}
        self.cats = {c["id"]: c for c in dataset.get("categories", [])}
        self.img_to_anns = {i: [] for i in self.imgs}
        for ann in dataset.get("annotations", []):
            self.img_to_anns.setdefault(ann["image_id"], []).append(ann)

    def img_ids(self):
        return sorted(self.imgs)

    def cat_ids(self):
        return sorted(self.cats)


def prepare(image, image_id, annotations):
    """One image's COCO annotation records -> the target dict (see the module docstring)."""
    w, h = image.size
    anno = [obj for obj in annotations if obj.get("iscrowd", 0) == 0]
    boxes = torch.as_tensor([obj["bbox"] for obj in anno], dtype=torch.float32).reshape(-1, 4)
    boxes[:, 2:] += boxes[:, :2]
    boxes[:, 0::2].clamp_(min=0, max=w)
    boxes[:, 1::2].clamp_(min=0, max=h)
    keep = (boxes[:, 3] > boxes[:, 1]) & (boxes[:, 2] > boxes[:, 0])
    return {
        "boxes": boxes[keep],
        "labels": torch.tensor([obj["category_id"] for obj in anno], dtype=torch.int64)[keep],
        "image_id": torch.tensor([image_id]),
        "area": torch.tensor([obj["area"] for obj in anno])[keep],
        "iscrowd": torch.tensor([obj.get("iscrowd", 0) for obj in anno])[keep],
        "orig_size": torch.as_tensor([int(h), int(w)]),
        "size": torch.as_tensor([int(h), int(w)]),
    }


class CocoDetection(torch.utils.data.Dataset):
    def __init__(self, img_folder, ann_file, transforms, device_plan=None):
        self.root = str(img_folder)
        self.coco = CocoGroundTruth(str(ann_file))
        self.ids = self.coco.img_ids()
        self._transforms = transforms
        self.device_plan = device_plan

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, idx):
        image_id = self.ids[idx]
        img = Image.open(os.path.join(self.root, self.coco.imgs[image_id]["file_name"])).convert("RGB")
        target = prepare(img, image_id, self.coco.img_to_anns[image_id])
        if self.device_plan is not None:
            return self.device_plan(img, target)
        if self._transforms is not None:
            img, target = self._transforms(img, target)
        return img, target


def coco_from_dataset(dataset):
    """The ground truth of a ``CocoDetection``, however many ``Subset`` wrappers sit on top of it."""
    while isinstance(dataset, torch.utils.data.Subset):
        dataset = dataset.dataset
    return dataset.coco
