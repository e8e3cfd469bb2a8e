"""COCO bounding-box average precision in numpy -- what the reference obtains from pycocotools through
``src/myrtle_vision/datasets/coco_eval.py`` -- with the reference's evaluator interface: ``update(res)``,
``synchronize_between_processes()``, ``accumulate()``, ``summarize()`` and ``coco_eval["bbox"].stats``.

The protocol (cocodataset.org, "Detection Evaluation"), as implemented here:

* Ground truth and detections are compared per image and per category.  A ground-truth box is IGNORED when it is a crowd
  region or when its annotated ``area`` lies outside the area range under evaluation; a detection's area is w * h.
* Per image and category the detections are ordered by descending score (stable) and cut at 100.  Overlap is
  intersection / union, except against a crowd region, where it is intersection / detection area.
* At each of the ten thresholds 0.50:0.05:0.95 the detections claim ground truth greedily in score order: a detection takes
  the not-yet-claimed box (a crowd region can be claimed repeatedly) of highest overlap >= the threshold, preferring any
  non-ignored box over every ignored one.  A detection matched to an ignored box is ignored; an unmatched detection whose own
  area lies outside the range is ignored; the rest are true or false positives.
* Over all evaluated images of a category the non-ignored detections (cut at maxDets 1 / 10 / 100 per image) are ordered by
  score, precision is made monotonically non-increasing from the right, and sampled at the 101 recall levels 0:0.01:1
  (0 where the recall is never reached).  Recall is the final true-positive count / non-ignored ground truth.
* A (category, area range) without non-ignored ground truth in the evaluated images takes no part in any mean (stored as -1);
  a statistic with no participant at all is -1.  The twelve ``stats``: AP@[.5:.95], AP@.5, AP@.75, AP small / medium / large
  (area < 32^2, 32^2..96^2, > 96^2) at maxDets 100; AR at maxDets 1, 10, 100; AR small / medium / large at maxDets 100.

This runs on the host: once per epoch, on a few thousand boxes, after the predictions have left the device anyway
(``PostProcess`` -- the softmax / arg-max / box scaling over all queries -- is the HIP part).  Only the images passed to
``update`` are evaluated, so a ``valid_subset`` scores against its own images.
"""
import numpy as np
import torch

from myrtle_vision.utils.utils import get_world_size, is_dist_avail_and_initialized

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)
RECALL_LEVELS = np.linspace(0.0, 1.0, 101)
MAX_DETS = (1, 10, 100)
AREA_RANGES = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))     # all, small, medium, large
AREA_NAMES = ("all", "small", "medium", "large")


def box_overlaps(dt, gt, crowd):
    """dt [D, 4], gt [G, 4] as (x, y, w, h); crowd bool [G] -> [D, G] overlaps (see the module docstring)."""
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    iw = np.minimum(dt[:, None, 0] + dt[:, None, 2], gt[None, :, 0] + gt[None, :, 2]) - np.maximum(dt[:, None, 0], gt[None, :, 0])
    ih = np.minimum(dt[:, None, 1] + dt[:, None, 3], gt[None, :, 1] + gt[None, :, 3]) - np.maximum(dt[:, None, 1], gt[None, :, 1])
    inter = np.clip(iw, 0.0, None) * np.clip(ih, 0.0, None)
    da, ga = (dt[:, 2] * dt[:, 3])[:, None], (gt[:, 2] * gt[:, 3])[None, :]
    union = np.where(np.asarray(crowd, bool)[None, :], da, da + ga - inter)
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


class BBoxEval:
    """Per-image matching records, their accumulation into precision / recall arrays and the twelve summary numbers."""

    def __init__(self, coco_gt):
        self.coco_gt = coco_gt
        self.cat_ids = coco_gt.cat_ids()
        self.eval_imgs = {}                                    # image id -> {(category index, area index): record}
        self.eval = None
        self.stats = None

    # ---- per image ----------------------------------------------------------------------------------------------
    def evaluate_image(self, img_id, boxes, scores, labels):
        """Detections of one image (boxes xywh) against its ground truth, for every category and area range."""
        boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
        scores, labels = np.asarray(scores, np.float64).reshape(-1), np.asarray(labels).reshape(-1)
        anns = self.coco_gt.img_to_anns.get(img_id, [])
        records = {}
        for k, cat in enumerate(self.cat_ids):
            g = [a for a in anns if a["category_id"] == cat]
            d = np.flatnonzero(labels == cat)
            if not g and d.size == 0:
                continue
            d = d[np.argsort(-scores[d], kind="stable")][:MAX_DETS[-1]]
            d_box, d_score = boxes[d], scores[d]
            d_area = d_box[:, 2] * d_box[:, 3]
            g_box = np.asarray([a["bbox"] for a in g], np.float64).reshape(-1, 4)
            g_area = np.asarray([a["area"] for a in g], np.float64)
            g_crowd = np.asarray([bool(a.get("iscrowd", 0)) for a in g], bool)
            overlaps = box_overlaps(d_box, g_box, g_crowd)
            for a, (lo, hi) in enumerate(AREA_RANGES):
                g_ignore = g_crowd | (g_area < lo) | (g_area > hi)
                order = np.argsort(g_ignore, kind="stable")                    # non-ignored ground truth is tried first
                matched, d_ignore = self._match(overlaps[:, order], g_ignore[order], g_crowd[order])
                d_ignore |= ~matched & ((d_area < lo) | (d_area > hi))[None, :]
                records[(k, a)] = {"scores": d_score, "matched": matched, "dt_ignore": d_ignore, "gt_ignore": g_ignore[order]}
        self.eval_imgs[img_id] = records

    @staticmethod
    def _match(overlaps, g_ignore, g_crowd):
        """Greedy claim of ground truth (columns, non-ignored first) by detections (rows, best score first) per threshold
        -> (matched bool [T, D], matched-to-ignored bool [T, D])."""
        D, G = overlaps.shape
        matched, to_ignored = np.zeros((len(IOU_THRESHOLDS), D), bool), np.zeros((len(IOU_THRESHOLDS), D), bool)
        for t, thr in enumerate(IOU_THRESHOLDS):
            taken = np.zeros(G, bool)
            for d in range(D):
                best, best_g = min(thr, 1 - 1e-10), -1
                for g in range(G):
                    if taken[g] and not g_crowd[g]:
                        continue
                    if best_g >= 0 and not g_ignore[best_g] and g_ignore[g]:
                        break                                   # a real match is never traded for an ignored box
                    if overlaps[d, g] < best:
                        continue
                    best, best_g = overlaps[d, g], g
                if best_g >= 0:
                    taken[best_g] = True
                    matched[t, d], to_ignored[t, d] = True, g_ignore[best_g]
        return matched, to_ignored

    # ---- over the images ----------------------------------------------------------------------------------------
    def accumulate(self):
        T, R, K, A, M = len(IOU_THRESHOLDS), len(RECALL_LEVELS), len(self.cat_ids), len(AREA_RANGES), len(MAX_DETS)
        precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
        img_ids = sorted(self.eval_imgs)
        for k in range(K):
            for a in range(A):
                recs = [self.eval_imgs[i][(k, a)] for i in img_ids if (k, a) in self.eval_imgs[i]]
                if not recs:
                    continue
                n_gt = int(sum((~r["gt_ignore"]).sum() for r in recs))
                if n_gt == 0:
                    continue
                for m, max_det in enumerate(MAX_DETS):
                    scores = np.concatenate([r["scores"][:max_det] for r in recs])
                    order = np.argsort(-scores, kind="stable")
                    matched = np.concatenate([r["matched"][:, :max_det] for r in recs], axis=1)[:, order]
                    ignored = np.concatenate([r["dt_ignore"][:, :max_det] for r in recs], axis=1)[:, order]
                    tp = np.cumsum(matched & ~ignored, axis=1, dtype=np.float64)
                    fp = np.cumsum(~matched & ~ignored, axis=1, dtype=np.float64)
                    for t in range(T):
                        rc = tp[t] / n_gt
                        pr = tp[t] / (tp[t] + fp[t] + np.spacing(1))
                        recall[t, k, a, m] = rc[-1] if rc.size else 0.0
                        pr = np.maximum.accumulate(pr[::-1])[::-1]           # best precision at this recall or beyond
                        at = np.searchsorted(rc, RECALL_LEVELS, side="left")
                        precision[t, :, k, a, m] = np.where(at < rc.size, np.append(pr, 0.0)[np.minimum(at, rc.size)], 0.0)
        self.eval = {"precision": precision, "recall": recall}

    def _mean(self, ap, iou=None, area="all", max_dets=100):
        a, m = AREA_NAMES.index(area), MAX_DETS.index(max_dets)
        s = self.eval["precision"][:, :, :, a, m] if ap else self.eval["recall"][:, :, a, m]
        if iou is not None:
            s = s[np.isclose(IOU_THRESHOLDS, iou)]
        s = s[s > -1]
        return float(s.mean()) if s.size else -1.0

    def summarize(self, verbose=True):
        if self.eval is None:
            raise RuntimeError("accumulate() first")
        rows = [(True, None, "all", 100), (True, 0.5, "all", 100), (True, 0.75, "all", 100), (True, None, "small", 100),
                (True, None, "medium", 100), (True, None, "large", 100), (False, None, "all", 1), (False, None, "all", 10),
                (False, None, "all", 100), (False, None, "small", 100), (False, None, "medium", 100), (False, None, "large", 100)]
        self.stats = np.array([self._mean(*r) for r in rows])
        if verbose:
            for (ap, iou, area, md), v in zip(rows, self.stats):
                name = "Average Precision  (AP)" if ap else "Average Recall     (AR)"
                rng = "0.50:0.95" if iou is None else f"{iou:0.2f}"
                print(f" {name} @[ IoU={rng:<9} | area={area:>6s} | maxDets={md:>3d} ] = {v:0.3f}")
        return self.stats


class CocoEvaluator:
    """``coco_gt``: a ``datasets.coco.CocoGroundTruth``; ``iou_types``: ("bbox",) -- masks and keypoints are out of scope."""

    def __init__(self, coco_gt, iou_types=("bbox",)):
        assert isinstance(iou_types, (list, tuple))
        if list(iou_types) != ["bbox"]:
            raise ValueError(f"only the 'bbox' evaluation is implemented, got {list(iou_types)}")
        self.coco_gt = coco_gt
        self.iou_types = list(iou_types)
        self.coco_eval = {"bbox": BBoxEval(coco_gt)}
        self.img_ids = []

    def update(self, predictions):
        """``predictions``: image id -> {"boxes": xyxy [N, 4] in original-image pixels, "scores": [N], "labels": [N]}
        (``PostProcess`` output).  An image id seen before is evaluated again and replaces its earlier record."""
        for img_id, pred in predictions.items():
            img_id = int(img_id)
            self.img_ids.append(img_id)
            if len(pred) == 0:
                self.coco_eval["bbox"].evaluate_image(img_id, np.zeros((0, 4)), np.zeros(0), np.zeros(0, np.int64))
                continue
            xyxy = torch.as_tensor(pred["boxes"]).detach().cpu().to(torch.float64).reshape(-1, 4).numpy()
            xywh = np.concatenate([xyxy[:, :2], xyxy[:, 2:] - xyxy[:, :2]], axis=1)
            self.coco_eval["bbox"].evaluate_image(img_id, xywh, torch.as_tensor(pred["scores"]).detach().cpu().numpy(),
                                                  torch.as_tensor(pred["labels"]).detach().cpu().numpy())

    def synchronize_between_processes(self):
        """Every rank ends up with the records of every image evaluated on any rank; an image seen by more than one rank
        (a padded shard) keeps the record of the lowest rank."""
        if not is_dist_avail_and_initialized() or get_world_size() == 1:
            return
        import torch.distributed as dist
        gathered = [None] * get_world_size()
        dist.all_gather_object(gathered, self.coco_eval["bbox"].eval_imgs)
        merged = {}
        for part in gathered:
            for img_id, rec in part.items():
                merged.setdefault(img_id, rec)
        self.coco_eval["bbox"].eval_imgs = merged
        self.img_ids = sorted(merged)

    def accumulate(self):
        self.coco_eval["bbox"].accumulate()

    def summarize(self, verbose=True):
        if verbose:
            print("IoU metric: bbox")
        self.coco_eval["bbox"].summarize(verbose)
