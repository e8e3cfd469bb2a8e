"""CPU: the detection data path -- transforms and their box arithmetic against formulas restated here and against recorded
outputs of the reference's own transforms, the padded collate, the COCO dataset reader on the synthetic directory, and the
numpy COCO bbox evaluator against closed forms and an independent brute-force restatement of the protocol."""
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from detection_data_samples import SAMPLES, cases, data_config, make_sample

F32 = np.float32


# ---- formulas, restated ---------------------------------------------------------------------------------------------
def size_rule(w, h, size, max_size):
    if max_size is not None and max(w, h) / min(w, h) * size > max_size:
        size = int(round(max_size * min(w, h) / max(w, h)))
    if min(w, h) == size:
        oh, ow = h, w
    elif w < h:
        oh, ow = int(size * h / w), size
    else:
        oh, ow = size, int(size * w / h)
    return oh // 16 * 16, ow // 16 * 16


def np_flip(b, w):
    return np.stack([F32(w) - b[:, 2], b[:, 1], F32(w) - b[:, 0], b[:, 3]], 1)


def np_crop(b, top, left, h, w):
    s = b - np.array([left, top, left, top], F32)
    s = np.maximum(np.minimum(s, np.array([w, h, w, h], F32)), F32(0))
    keep = (s[:, 2] > s[:, 0]) & (s[:, 3] > s[:, 1])
    return s[keep], keep


def np_scale(b, rw, rh):
    return b * np.array([rw, rh, rw, rh]).astype(F32)


def np_normalize(b, w, h):
    c = np.stack([(b[:, 0] + b[:, 2]) / F32(2), (b[:, 1] + b[:, 3]) / F32(2), b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)
    return c / np.array([w, h, w, h], F32)


def _boxes(t):
    return t["boxes"].numpy().astype(F32)


@pytest.mark.parametrize("w,h,size,max_size,expected", [
    (500, 400, 320, 533, (320, 400)), (400, 500, 320, 533, (400, 320)), (480, 480, 320, 533, (320, 320)),
    (1000, 800, 800, 1333, (800, 992)),                     # short side already the size: sides kept, floored to 16
    (1000, 400, 800, 1333, (528, 1328)),                    # clamp: 2.5 * 800 > 1333 -> size 533 -> (533, 1332) -> floored
    (37, 53, 16, None, (16, 16)), (333, 500, 608, 1013, (912, 608))])
def test_size_rule(w, h, size, max_size, expected):
    from myrtle_vision.datasets.detection_transforms import output_size
    assert size_rule(w, h, size, max_size) == expected
    assert output_size((w, h), size, max_size) == expected


@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_each_transform_follows_its_formula(name):
    from myrtle_vision.datasets import detection_transforms as T
    img, target = make_sample(name)
    w, h = img.size
    b0 = _boxes(target)
    # flip
    random.seed(1)
    flipped_expected = random.random() < 0.5
    random.seed(1)
    out, t = T.RandomHorizontalFlip()(img, target)
    assert np.array_equal(_boxes(t), np_flip(b0, w) if flipped_expected else b0)
    assert np.array_equal(np.asarray(out), np.asarray(img)[:, ::-1] if flipped_expected else np.asarray(img))
    # resize: the drawn scale, the size rule, ratios rounded to fp32 once, area by their product
    sizes, max_size = [96, 128, min(w, h)], 200
    for seed in range(4):
        random.seed(seed)
        size = random.choice(sizes)
        random.seed(seed)
        out, t = T.RandomResize(sizes, max_size)(img, target)
        oh, ow = size_rule(w, h, size, max_size)
        assert out.size == (ow, oh) and t["size"].tolist() == [oh, ow]
        assert np.array_equal(_boxes(t), np_scale(b0, ow / w, oh / h))
        assert np.array_equal(t["area"].numpy(), target["area"].numpy() * F32((ow / w) * (oh / h)))
    # crop: sizes from random.randint, the offset from torch.randint (top, then left); boxes shifted, clamped, dropped
    cut = removed = False
    for seed in range(6):
        random.seed(seed)
        torch.manual_seed(seed)
        cw, ch = random.randint(100, min(w, 300)), random.randint(100, min(h, 300))
        top, left = int(torch.randint(0, h - ch + 1, (1,))), int(torch.randint(0, w - cw + 1, (1,)))
        random.seed(seed)
        torch.manual_seed(seed)
        out, t = T.RandomSizeCrop(100, 300)(img, target)
        exp, keep = np_crop(b0, top, left, ch, cw)
        assert out.size == (cw, ch) and t["size"].tolist() == [ch, cw]
        assert np.array_equal(np.asarray(out), np.asarray(img)[top:top + ch, left:left + cw])
        assert np.array_equal(_boxes(t), exp) and t["labels"].tolist() == target["labels"][torch.from_numpy(keep)].tolist()
        assert np.array_equal(t["area"].numpy(), (exp[:, 2] - exp[:, 0]) * (exp[:, 3] - exp[:, 1]))
        assert len(t["iscrowd"]) == len(exp)
        removed |= bool((~keep).any())
        shifted = (b0 - np.array([left, top, left, top], F32))[keep]
        cut |= bool((shifted != exp).any())
    if len(b0):
        assert cut and removed, "the crops of this test must both cut and remove boxes"
    # normalize
    out, t = T.Compose([T.ToTensor(), T.Normalize([0.5, 0.4, 0.3], [0.5, 0.25, 0.2])])(img, target)
    assert np.array_equal(_boxes(t), np_normalize(b0, w, h))
    a = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float() / 255
    assert torch.equal(out, (a - torch.tensor([0.5, 0.4, 0.3]).view(3, 1, 1)) / torch.tensor([0.5, 0.25, 0.2]).view(3, 1, 1))


def _replay(section, img, target, seed):
    """The chain of the shipped data config, restated: flip?, then select(resize | resize-crop-resize), then normalize."""
    from PIL import Image
    random.seed(seed)
    torch.manual_seed(seed)
    w, h = img.size
    b, labels = _boxes(target), target["labels"].numpy()
    resize_keys = [k for k in section if k.endswith("RandomResize")]

    def do_resize(img, b, spec):
        scales = spec["scales"]
        max_size = None if spec.get("max_size_ratio") is None else max(scales) * spec["max_size_ratio"][0] // spec["max_size_ratio"][1]
        w, h = img.size
        oh, ow = size_rule(w, h, random.choice(scales), max_size)
        return img.resize((ow, oh), Image.Resampling.BILINEAR), np_scale(b, ow / w, oh / h)

    if "RandomHorizontalFlip" in section and random.random() < 0.5:
        img, b = img.transpose(Image.Transpose.FLIP_LEFT_RIGHT), np_flip(b, w)
    if "RandomSelect" in section:
        sel = section["RandomSelect"]
        if random.random() < 0.5:
            img, b = do_resize(img, b, sel["RandomResize"])
        else:
            c = sel["Compose"]
            img, b = do_resize(img, b, c["PreRandomResize"])
            lo, hi = c["RandomSizeCrop"]
            cw, ch = random.randint(lo, min(img.width, hi)), random.randint(lo, min(img.height, hi))
            top = left = 0
            if (ch, cw) != (img.height, img.width):
                top, left = int(torch.randint(0, img.height - ch + 1, (1,))), int(torch.randint(0, img.width - cw + 1, (1,)))
            img = img.crop((left, top, left + cw, top + ch))
            b, keep = np_crop(b, top, left, ch, cw)
            labels = labels[keep]
            img, b = do_resize(img, b, c["PostRandomResize"])
    for k in resize_keys:
        img, b = do_resize(img, b, section[k])
    n = section["Normalize"]
    a = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float() / 255
    a = (a - torch.tensor(n["Mean"]).view(3, 1, 1)) / torch.tensor(n["Std"]).view(3, 1, 1)
    return a, np_normalize(b, img.width, img.height), labels


@pytest.fixture(scope="module")
def chain_outputs():
    from myrtle_vision.datasets.detection_transforms import from_config
    cfg, out = data_config(), {}
    for chain, name, seed in cases():
        img, target = make_sample(name)
        random.seed(seed)
        torch.manual_seed(seed)
        out[(chain, name, seed)] = from_config(cfg[chain])(img, target)
    return out


def test_from_config_chains_follow_the_restated_formulas(chain_outputs):
    cfg = data_config()
    for (chain, name, seed), (img, t) in chain_outputs.items():
        a, b, labels = _replay(cfg[chain], *make_sample(name), seed)
        assert torch.equal(img, a), (chain, name, seed)
        assert t["labels"].tolist() == labels.tolist() and t["size"].tolist() == list(a.shape[-2:])
        # same operations in the same order in fp32: exact
        assert np.array_equal(_boxes(t), b), (chain, name, seed)
        assert a.shape[-1] % 16 == 0 and a.shape[-2] % 16 == 0


def test_from_config_chains_reproduce_the_reference_fixtures(chain_outputs):
    """tests/golden/detection_transforms_ref.json: the reference's own transforms on the same samples and seeds."""
    rows = json.load(open(os.path.join(GOLDEN, "detection_transforms_ref.json")))
    assert len(rows) == len(chain_outputs) == len(cases())
    two_stage = 0
    for r in rows:
        img, t = chain_outputs[(r["chain"], r["sample"], r["seed"])]
        assert list(img.shape) == r["shape"] and t["size"].tolist() == r["size"]
        assert t["labels"].tolist() == r["labels"]
        assert t["boxes"].double().tolist() == r["boxes"] and t["area"].double().tolist() == r["area"]
        assert float(img.double().sum()) == r["pixel_sum"]
        two_stage += len(r["labels"]) < len(SAMPLES[r["sample"]][2])
    assert two_stage >= 3                                       # the crop branch was taken and removed boxes


def test_from_config_ignores_unknown_ops_and_keeps_key_order():
    from myrtle_vision.datasets import detection_transforms as T
    c = T.from_config({"RandomPad": 3, "PostRandomResize": {"scales": [32]}, "RandomHorizontalFlip": None,
                       "Normalize": {"Mean": [0, 0, 0], "Std": [1, 1, 1]}})
    assert [type(t).__name__ for t in c.transforms] == ["RandomResize", "RandomHorizontalFlip", "ToTensor", "Normalize"]
    c = T.from_config({"RandomResize": {"scales": [400, 608], "max_size_ratio": [1333, 800]}})
    assert c.transforms[0].max_size == 608 * 1333 // 800


def test_collate_pads_with_zeros_and_masks_the_padding():
    from myrtle_vision.datasets.detection_transforms import NestedTensor, collate_fn
    shapes = [(3, 16, 48), (3, 32, 16), (3, 32, 48), (3, 17, 5)]
    imgs = [torch.full(s, float(i + 1)) for i, s in enumerate(shapes)]
    nested, targets = collate_fn([(im, {"k": i}) for i, im in enumerate(imgs)])
    assert isinstance(nested, NestedTensor) and targets == tuple({"k": i} for i in range(4))
    t, m = nested.decompose()
    assert t.shape == (4, 3, 32, 48) and m.shape == (4, 32, 48) and m.dtype == torch.bool
    for i, (_, h, w) in enumerate(shapes):
        assert torch.equal(t[i, :, :h, :w], imgs[i])
        expect = torch.ones(32, 48, dtype=torch.bool)
        expect[:h, :w] = False
        assert torch.equal(m[i], expect)
        assert float(t[i][:, expect].abs().sum()) == 0.0


# ---- dataset ---------------------------------------------------------------------------------------------------------
def test_coco_detection_reads_the_synthetic_directory(tmp_path):
    from torch.utils.data import Subset
    from myrtle_vision.datasets.coco import CocoDetection, coco_from_dataset
    from myrtle_vision.datasets.synthetic import make_dior_coco
    root = make_dior_coco(str(tmp_path / "DIOR-COCO"))
    ann = json.load(open(os.path.join(root, "annotations", "train.json")))
    assert len(ann["categories"]) == 20 and len({(i["height"], i["width"]) for i in ann["images"]}) >= 3
    ds = CocoDetection(os.path.join(root, "train"), os.path.join(root, "annotations", "train.json"), None)
    assert len(ds) == 8 and coco_from_dataset(Subset(Subset(ds, [0, 1]), [0])) is ds.coco
    img, t = ds[0]
    w, h = img.size
    recs = [a for a in ann["annotations"] if a["image_id"] == ds.ids[0]]
    assert any(a["iscrowd"] for a in recs) and any(a["bbox"][2] == 0 for a in recs)
    assert any(a["bbox"][0] + a["bbox"][2] > w for a in recs)
    kept = [a for a in recs if not a["iscrowd"] and a["bbox"][2] > 0 and a["bbox"][3] > 0]
    assert len(kept) == len(recs) - 2                           # the crowd region and the zero-width box are gone
    assert set(t) == {"boxes", "labels", "image_id", "area", "iscrowd", "orig_size", "size"}
    assert t["boxes"].dtype == torch.float32 and t["boxes"].shape == (len(kept), 4) and t["labels"].dtype == torch.int64
    assert t["labels"].tolist() == [a["category_id"] for a in kept] and t["iscrowd"].tolist() == [0] * len(kept)
    assert t["image_id"].tolist() == [ds.ids[0]] and t["orig_size"].tolist() == [h, w] == t["size"].tolist()
    expect = torch.tensor([[a["bbox"][0], a["bbox"][1], min(a["bbox"][0] + a["bbox"][2], w), min(a["bbox"][1] + a["bbox"][3], h)]
                           for a in kept], dtype=torch.float32)
    assert torch.equal(t["boxes"], expect) and float(t["boxes"][:, 2].max()) == w  # xywh -> xyxy, clamped to the frame
    assert t["area"].tolist() == [a["area"] for a in kept]
    assert len(ds.coco.img_to_anns[ds.ids[0]]) == len(recs)                        # the evaluator still sees the crowd region


# ---- evaluator -------------------------------------------------------------------------------------------------------
def _gt(images, anns, cats=(0, 1, 2)):
    from myrtle_vision.datasets.coco import CocoGroundTruth
    return CocoGroundTruth(dataset={
        "images": [{"id": i, "file_name": f"{i}.jpg", "height": 400, "width": 400} for i in images],
        "categories": [{"id": c, "name": str(c)} for c in cats],
        "annotations": [{"id": n + 1, "image_id": a[0], "category_id": a[1], "bbox": list(a[2]), "area": float(a[2][2] * a[2][3]),
                         "iscrowd": a[3] if len(a) > 3 else 0} for n, a in enumerate(anns)]})


def _run(gt, dets):
    """dets: image id -> list of (category, xywh, score)."""
    from myrtle_vision.datasets.coco_eval import CocoEvaluator
    ev = CocoEvaluator(gt, ["bbox"])
    res = {}
    for i, d in dets.items():
        b = torch.tensor([x[1] for x in d], dtype=torch.float64).reshape(-1, 4)
        res[i] = {"boxes": torch.cat([b[:, :2], b[:, :2] + b[:, 2:]], 1), "scores": torch.tensor([x[2] for x in d]),
                  "labels": torch.tensor([x[0] for x in d], dtype=torch.int64)}
    ev.update(res)
    ev.synchronize_between_processes()
    ev.accumulate()
    ev.summarize(verbose=False)
    return ev.coco_eval["bbox"].stats


_ANNS = [(1, 0, (10, 10, 20, 20)), (1, 0, (100, 100, 50, 50)), (1, 1, (200, 200, 120, 120)), (2, 0, (30, 40, 60, 60)),
         (2, 1, (5, 5, 10, 10))]


def test_evaluator_closed_forms():
    gt = _gt([1, 2], _ANNS)                                     # category 2 has no ground truth: excluded from every mean
    perfect = {i: [(a[1], a[2], 0.9 - 0.1 * n) for n, a in enumerate(_ANNS) if a[0] == i] for i in (1, 2)}
    stats = _run(gt, perfect)
    assert stats.shape == (12,)
    # small: 20x20, 10x10; medium: 50x50, 60x60; large: 120x120 -> every range has instances.  AR@1: one detection per image and
    # category: category 0 finds 1 of 2 in image 1 and 1 of 1 in image 2 (2 of 3); category 1 finds 2 of 2
    expected = np.ones(12)
    expected[6] = (2 / 3 + 1.0) / 2
    assert np.allclose(stats, expected, atol=1e-12)
    assert np.array_equal(_run(gt, {1: [], 2: []}), np.zeros(12))
    # detections of a category without ground truth change nothing; a GT-free evaluation is -1 everywhere
    noise = {i: d + [(2, (50, 50, 30, 30), 0.99)] for i, d in perfect.items()}
    assert np.allclose(_run(gt, noise), expected, atol=1e-12)
    assert np.array_equal(_run(_gt([1], []), {1: [(0, (1, 1, 5, 5), 0.5)]}), -np.ones(12))


def test_evaluator_hand_computed_two_image_case():
    """Category 0 only.  Image 1: ground truth A = (0, 0, 100, 100) and B = (200, 200, 100, 100); image 2: C = (0, 0, 50, 50).
    Detections by score: 0.9 = A exactly (TP at every threshold); 0.8 in image 2 = (0, 0, 50, 41): IoU with C 0.82 (TP up to
    0.80, FP at 0.85+); 0.7 in image 1 = (300, 0, 50, 50): FP; 0.6 = B cut to (200, 200, 100, 82): IoU 0.82.
    Thresholds <= 0.80 (7 of 10): TP, TP, FP, TP -> precision envelope 1, 1, 3/4, 3/4 at recalls 1/3, 2/3, 2/3, 1:
    AP = (67 * 1 + 34 * 0.75) / 101.  Thresholds >= 0.85 (3 of 10): TP, FP, FP, FP -> recall 1/3 at precision 1:
    AP = 34 / 101."""
    gt = _gt([1, 2], [(1, 0, (0, 0, 100, 100)), (1, 0, (200, 200, 100, 100)), (2, 0, (0, 0, 50, 50))], cats=(0,))
    dets = {1: [(0, (0, 0, 100, 100), 0.9), (0, (300, 0, 50, 50), 0.7), (0, (200, 200, 100, 82), 0.6)],
            2: [(0, (0, 0, 50, 41), 0.8)]}
    stats = _run(gt, dets)
    lo, hi = (67 + 34 * 0.75) / 101, 34 / 101
    assert abs(stats[0] - (7 * lo + 3 * hi) / 10) < 1e-12
    assert abs(stats[1] - lo) < 1e-12 and abs(stats[2] - lo) < 1e-12          # IoU 0.50 and 0.75
    assert abs(stats[8] - (7 * 1.0 + 3 * (1 / 3)) / 10) < 1e-12              # AR@100
    assert abs(stats[6] - (7 * (2 / 3) + 3 * (1 / 3)) / 10) < 1e-12          # AR@1: the best detection per image only
    assert stats[3] == -1.0 and stats[9] == -1.0                             # no small ground truth (50^2 = 2500 is medium)


def _brute_force_stats(images, cats, anns, dets):
    """The COCO bbox protocol with nested loops and python floats only; ``anns`` (image, cat, xywh, crowd), ``dets`` image ->
    [(cat, xywh, score)]."""
    thresholds = [0.5 + 0.05 * i for i in range(10)]
    ranges = [(0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10)]

    def overlap(d, g, crowd):
        iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
        ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
        inter = max(iw, 0.0) * max(ih, 0.0)
        return inter / (d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - inter)

    def ap_ar(ti, ri, max_det):
        aps, ars = [], []
        for cat in cats:
            lo, hi = ranges[ri]
            rows, n_gt = [], 0                                  # rows: (score, is_tp, ignored)
            for img in images:
                gts = [(a[2], bool(a[3]), bool(a[3]) or not (lo <= a[2][2] * a[2][3] <= hi)) for a in anns if a[0] == img and a[1] == cat]
                gts = [g for g in gts if not g[2]] + [g for g in gts if g[2]]
                n_gt += sum(1 for g in gts if not g[2])
                ds = sorted([d for d in dets.get(img, []) if d[0] == cat], key=lambda d: -d[2])[:100]
                taken = [False] * len(gts)
                per_image = []
                for d in ds:
                    best, which = min(thresholds[ti], 1 - 1e-10), -1
                    for gi, (gbox, crowd, ign) in enumerate(gts):
                        if taken[gi] and not crowd:
                            continue
                        if which >= 0 and not gts[which][2] and ign:
                            break
                        o = overlap(d[1], gbox, crowd)
                        if o < best:
                            continue
                        best, which = o, gi
                    if which >= 0:
                        taken[which] = True
                        per_image.append((d[2], True, gts[which][2]))
                    else:
                        per_image.append((d[2], False, not (lo <= d[1][2] * d[1][3] <= hi)))
                rows += per_image[:max_det]
            if n_gt == 0:
                continue
            rows.sort(key=lambda r: -r[0])
            tp = fp = 0
            curve = []
            for _, is_tp, ign in rows:
                if not ign:
                    tp, fp = tp + is_tp, fp + (not is_tp)
                curve.append((tp / n_gt, tp / (tp + fp + np.spacing(1))))
            ars.append(curve[-1][0] if curve else 0.0)
            total = 0.0
            for r in range(101):
                level = float(np.linspace(0.0, 1.0, 101)[r])
                total += max([p for rc, p in curve if rc >= level], default=0.0)
            aps.append(total / 101)
        return aps, ars

    def mean_over(kind, tis, ri, max_det):
        vals = []
        for ti in tis:
            vals += ap_ar(ti, ri, max_det)[kind]
        return sum(vals) / len(vals) if vals else -1.0

    every = list(range(10))
    return [mean_over(0, every, 0, 100), mean_over(0, [0], 0, 100), mean_over(0, [5], 0, 100), mean_over(0, every, 1, 100),
            mean_over(0, every, 2, 100), mean_over(0, every, 3, 100), mean_over(1, every, 0, 1), mean_over(1, every, 0, 10),
            mean_over(1, every, 0, 100), mean_over(1, every, 1, 100), mean_over(1, every, 2, 100), mean_over(1, every, 3, 100)]


def test_evaluator_agrees_with_a_brute_force_restatement():
    rng = np.random.default_rng(5)
    images, cats = [3, 5, 8, 13, 21], (0, 1, 2, 3)             # category 3 gets detections but no ground truth
    anns, dets = [], {i: [] for i in images}
    sides = [(8, 30), (35, 90), (100, 180)]                    # small, medium, large
    for n, img in enumerate(images):
        for j in range(7):
            lo, hi = sides[(n + j) % 3]
            w, h = rng.uniform(lo, hi, 2)
            x, y = rng.uniform(0, 400 - w), rng.uniform(0, 400 - h)
            cat = int(rng.integers(0, 3))
            anns.append((img, cat, (float(x), float(y), float(w), float(h)), 0))
            for _ in range(int(rng.integers(0, 4))):           # jittered copies: overlaps on both sides of the thresholds
                jx, jy, jw, jh = rng.normal(0, 0.12, 4)
                dets[img].append((cat if rng.random() < 0.85 else int(rng.integers(0, 4)),
                                  (float(x + jx * w), float(y + jy * h), float(w * (1 + jw)), float(h * (1 + jh)))))
        for _ in range(3):                                     # strays
            w, h = rng.uniform(8, 150, 2)
            dets[img].append((int(rng.integers(0, 4)), (float(rng.uniform(0, 300)), float(rng.uniform(0, 300)), float(w), float(h))))
    anns.append((5, 1, (50.0, 50.0, 200.0, 200.0), 1))         # one crowd region, with two detections inside it
    dets[5] += [(1, (60.0, 60.0, 40.0, 40.0)), (1, (120.0, 130.0, 70.0, 50.0))]
    total = sum(len(d) for d in dets.values())
    scores = rng.permutation(total) / total + 0.001            # no duplicate scores
    k = 0
    for img in images:
        for j, d in enumerate(dets[img]):
            dets[img][j] = (d[0], d[1], float(scores[k]))
            k += 1
    areas = [a[2][2] * a[2][3] for a in anns]
    assert min(areas) < 1024 < sorted(areas)[len(areas) // 2] and max(areas) > 9216 and total > 40
    stats = _run(_gt(images, anns, cats), dets)
    expected = _brute_force_stats(images, cats, anns, dets)
    assert np.all(stats > 0) and np.all(stats < 1)             # a case in which every statistic is informative
    assert np.abs(stats - np.array(expected)).max() <= 1e-12, (stats, expected)


def test_evaluator_scores_only_the_images_it_was_given():
    gt = _gt([1, 2], _ANNS)
    only_1 = {1: [(a[1], a[2], 0.9) for a in _ANNS if a[0] == 1]}
    assert _run(gt, only_1)[0] == 1.0                           # image 2's ground truth is not counted as missed


# ---- two ranks over gloo ---------------------------------------------------------------------------------------------
def _sync_worker(rank, world, port, tmpdir):
    import torch.distributed as dist
    from myrtle_vision.datasets.coco_eval import CocoEvaluator
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    gt = _gt([1, 2, 3], _SYNC_ANNS)
    ev = CocoEvaluator(gt, ["bbox"])
    mine = {1: [1, 2], 0: [3, 1]}[rank]                         # image 1 on both ranks, as a padded shard would have it
    res = {}
    for i in mine:
        d = _SYNC_DETS[i]
        b = torch.tensor([x[1] for x in d], dtype=torch.float64).reshape(-1, 4)
        res[i] = {"boxes": torch.cat([b[:, :2], b[:, :2] + b[:, 2:]], 1), "scores": torch.tensor([x[2] for x in d]),
                  "labels": torch.tensor([x[0] for x in d], dtype=torch.int64)}
    ev.update(res)
    ev.synchronize_between_processes()
    ev.accumulate()
    ev.summarize(verbose=False)
    np.save(os.path.join(tmpdir, f"stats{rank}.npy"), ev.coco_eval["bbox"].stats)
    dist.destroy_process_group()


_SYNC_ANNS = [(1, 0, (0, 0, 100, 100)), (2, 0, (10, 10, 40, 40)), (2, 1, (100, 100, 120, 120)), (3, 1, (5, 5, 20, 20))]
_SYNC_DETS = {1: [(0, (0, 0, 100, 90), 0.9), (1, (0, 0, 10, 10), 0.3)], 2: [(0, (10, 10, 40, 40), 0.8), (1, (100, 100, 120, 100), 0.7)],
              3: [(1, (5, 5, 20, 20), 0.6), (0, (50, 50, 20, 20), 0.95)]}


def test_synchronize_between_two_ranks_over_gloo(tmp_path):
    import torch.multiprocessing as mp
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_sync_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    s0, s1 = np.load(tmp_path / "stats0.npy"), np.load(tmp_path / "stats1.npy")
    single = _run(_gt([1, 2, 3], _SYNC_ANNS), _SYNC_DETS)
    assert np.array_equal(s0, s1) and np.array_equal(s0, single) and 0 < single[0] < 1


# ---- the device plan's tables, without a device ------------------------------------------------------------------------
def _resample_stage(src, p, suffix=""):
    """numpy restatement of the ragged kernels' arithmetic for one stage: per output pixel the horizontal taps (22-bit
    coefficients, + 2^21, >> 22, clipped to uint8), then the vertical taps alike; zero outside the sample's extent."""
    kh, bh, kv, bv = (p[k + suffix].numpy().astype(np.int64) for k in ("kh", "bh", "kv", "bv"))
    ext, src = p["ext" + suffix].numpy(), src.astype(np.int64)
    B, oh, ow = kv.shape[0], kv.shape[1], kh.shape[1]
    out, inside = np.zeros((B, oh, ow, 3), np.int64), np.zeros((B, oh, ow), bool)
    for b in range(B):
        eh, ew = ext[b]
        rows = np.zeros((src.shape[1], ew, 3), np.int64)
        for x in range(ew):
            x0, n = bh[b, x]
            rows[:, x] = np.clip(((1 << 21) + (src[b, :, x0:x0 + n] * kh[b, x, :n, None]).sum(1)) >> 22, 0, 255)
        for y in range(eh):
            y0, n = bv[b, y]
            out[b, y, :ew] = np.clip(((1 << 21) + (rows[y0:y0 + n] * kv[b, y, :n, None, None]).sum(0)) >> 22, 0, 255)
        inside[b, :eh, :ew] = True
    return out, inside


def test_device_plan_tables_reproduce_the_host_chain_under_the_kernel_arithmetic():
    """DetectionDevicePlan on the worker: the same draws and targets as the host chain, and tables that -- resampled with the
    kernel's integer arithmetic, restated above -- give the host batch bit for bit: flips folded into the taps, crops as table
    windows, two resamplings with the uint8 image in between, batches that mix one- and two-resampling samples."""
    from PIL import Image
    from myrtle_vision.datasets.detection_transforms import collate_fn, from_config
    from myrtle_vision.datasets.device_transforms import DetectionDevicePlan
    mean, std = [0.5, 0.4, 0.3], [0.5, 0.25, 0.2]
    train = {"RandomHorizontalFlip": None,
             "RandomSelect": {"RandomResize": {"scales": [16, 32, 48, 64, 96], "max_size_ratio": [4, 3]},
                              "Compose": {"PreRandomResize": {"scales": [48, 64, 80]}, "RandomSizeCrop": [32, 64],
                                          "PostRandomResize": {"scales": [32, 48, 96], "max_size_ratio": [4, 3]}}},
             "Normalize": {"Mean": mean, "Std": std}}
    val = {"RandomResize": {"scales": [48], "max_size_ratio": [3, 2]}, "Normalize": {"Mean": mean, "Std": std}}
    rng = np.random.default_rng(0)
    frames = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in ((37, 53), (64, 48), (80, 80), (96, 40))]

    def target(img):
        w, h = img.size
        b = torch.tensor([[1.0, 2.0, w / 2, h / 2], [w / 3, h / 4, w - 1.0, h - 2.0]])
        return {"boxes": b, "labels": torch.tensor([1, 2]), "area": (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]),
                "iscrowd": torch.zeros(2, dtype=torch.int64), "size": torch.tensor([h, w]), "orig_size": torch.tensor([h, w])}

    stages = set()
    for section, seeds in ((val, (0,)), (train, (0, 1, 2, 3))):
        host_chain, plan = from_config(section), DetectionDevicePlan(section)
        for seed in seeds:
            random.seed(seed)
            torch.manual_seed(seed)
            host, host_targets = collate_fn([host_chain(f, target(f)) for f in frames])
            random.seed(seed)
            torch.manual_seed(seed)
            samples = [plan(f, target(f)) for f in frames]
            stages |= {"kh1" in s[0] for s in samples}
            packed, targets = plan.collate(samples)
            src = packed["raw"].numpy()
            if "kh1" in packed:
                src = _resample_stage(src, packed, "1")[0]
            px, inside = _resample_stage(src, packed)
            m, s = (torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1) for v in packed["norm"].tolist())
            img = (torch.from_numpy(px.astype(np.float32)).permute(0, 3, 1, 2) / 255 - m) / s
            img = torch.where(torch.from_numpy(inside)[:, None], img, torch.zeros(()))
            assert torch.equal(img, host.tensors) and torch.equal(torch.from_numpy(~inside), host.mask), (section is val, seed)
            for a, b in zip(targets, host_targets):
                assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)
    assert stages == {False, True}


def test_device_plan_collate_refuses_mixed_normalisation():
    """One launch takes one mean / std: samples of chains that normalise differently must not share a batch."""
    from PIL import Image
    from myrtle_vision.datasets.device_transforms import DetectionDevicePlan
    frame = Image.fromarray(np.random.default_rng(0).integers(0, 256, (40, 56, 3), dtype=np.uint8))
    target = lambda: {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64), "area": torch.zeros(0),
                      "iscrowd": torch.zeros(0, dtype=torch.int64)}
    section = lambda std: {"RandomResize": {"scales": [32]}, "Normalize": {"Mean": [0.5] * 3, "Std": [std] * 3}}
    a, b = DetectionDevicePlan(section(0.5)), DetectionDevicePlan(section(0.25))
    packed, _ = a.collate([a(frame, target()), a(frame, target())])
    assert packed["norm"].tolist() == [[0.5] * 3, [0.5] * 3]
    with pytest.raises(ValueError, match="share the normalisation"):
        a.collate([a(frame, target()), b(frame, target())])


def test_shipped_configs_are_in_the_schema_the_loop_reads():
    """detection/{data,train}_configs: both chains build on the host and as device plans, and every key the optimizer, the
    criterion weights and the dataset factory read is present."""
    from myrtle_vision.datasets.detection_transforms import from_config
    from myrtle_vision.datasets.device_transforms import DetectionDevicePlan
    from myrtle_vision.utils.models import get_optimizer_args
    root = os.path.join(os.path.dirname(GOLDEN), os.pardir, "detection")
    data = json.load(open(os.path.join(root, "data_configs", "data_config.json")))
    for ops_ in ("transform_ops_train", "transform_ops_val"):
        from_config(data[ops_])
        DetectionDevicePlan(data[ops_])
    for split in ("train", "valid", "test"):
        assert isinstance(data[f"{split}_images"], str) and data[f"{split}_annotations"].endswith(".json")
    assert data["number_of_classes"] == 20 and "dataset_path" in data
    for name in ("tiny", "small", "base"):
        cfg = json.load(open(os.path.join(root, "train_configs", f"yolos_{name}.json")))
        t, v = cfg["train_config"], cfg["vit_config"]
        get_optimizer_args(t)
        assert all(t[k] > 0 for k in ("loss_ce", "loss_bbox", "loss_giou", "eos_coef"))
        assert t["global_batch_size"] % t["local_batch_size"] == 0 and t["device_transforms"] is True
        assert v["decoder"] == "detection" and v["embed_dim"] % v["heads"] == 0 and v["num_det_tokens"] == 100
        assert os.path.exists(os.path.join(root, cfg["data_config_path"]))
