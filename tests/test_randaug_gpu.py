"""RandAugment on the device: mv_randaug_stats / mv_randaug_apply against the direct Pillow call of every op, and DevicePlan's
whole chain against the host chain of datasets/transforms.py.  Every comparison is exact; dst, the tables and the means sit
between guard zones and src is checked to be intact."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

import randaug_ref as R
from randaug_ref import BIC, BIL, Guarded

pytestmark = pytest.mark.gpu

GROUPS = {"tables": lambda c: c[0] not in R.GEOMETRIC and c[0] not in R.ENHANCE,
          "enhance": lambda c: c[0] in R.ENHANCE,
          "bilinear": lambda c: c[0] in R.GEOMETRIC and c[2] == BIL,
          "bicubic": lambda c: c[0] in R.GEOMETRIC and c[2] == BIC}


def _batch(h, w):
    """7 images: the five kinds + two more draws of noise."""
    return np.stack(R.images(h, w) + [R.images(h, w, seed=s)[0] for s in (1, 2)])


def _run_slot(ops, G, src, op, par, slot, fill=R.FILL):
    """One slot through both entry points into guarded arrays -> dst (device)."""
    B = src.shape[0]
    tables, mean, dst = G.new((B, 3, 256), torch.uint8), G.new((B,), torch.int32), G.new(tuple(src.shape), torch.uint8)
    ops.randaug_stats(src, op, slot, tables, mean)
    out = ops.randaug_apply(src, op, par, slot, tables, mean, fill, out=dst)
    assert out.data_ptr() == dst.data_ptr()
    return dst


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("h,w", R.SIZES)
def test_every_op_equals_the_pillow_call(h, w, group):
    from myrtle_vision.hip import ops
    host = _batch(h, w)
    pil = [Image.fromarray(a) for a in host]
    src = torch.from_numpy(host).cuda()
    cases = [c for c in R.op_cases(h, w) if GROUPS[group](c)]
    assert cases
    G = Guarded(torch)
    results = []
    for case in cases:
        o, p = R.fields([case], w, h)
        op = torch.from_numpy(np.repeat(o[None], len(host), 0)).cuda()
        par = torch.from_numpy(np.repeat(p[None], len(host), 0)).cuda()
        results.append(_run_slot(ops, G, src, op, par, 0))
    torch.cuda.synchronize()
    G.check()
    assert np.array_equal(src.cpu().numpy(), host)
    for case, dst in zip(cases, results):
        got = dst.cpu().numpy()
        for i, img in enumerate(pil):
            assert np.array_equal(got[i], np.asarray(R.pillow_op(img, *case))), (case, i)


def test_autocontrast_at_every_range():
    from myrtle_vision.hip import ops
    host = np.stack(R.autocontrast_images())
    assert host.shape == (255, 16, 16, 3)
    src = torch.from_numpy(host).cuda()
    o, p = R.fields([("AutoContrast", None, None)], 16, 16)
    G = Guarded(torch)
    dst = _run_slot(ops, G, src, torch.from_numpy(np.repeat(o[None], 255, 0)).cuda(), torch.from_numpy(np.repeat(p[None], 255, 0)).cuda(), 0)
    got = dst.cpu().numpy()
    G.check()
    for i, a in enumerate(host):
        assert np.array_equal(got[i], np.asarray(R.pillow_op(Image.fromarray(a), "AutoContrast"))), i + 1


def test_mixed_batch_of_three_slots():
    """B = 19, every sample its own sequence of 3 slots (skipped slots and the same op twice among them), 37 x 53."""
    from myrtle_vision.hip import ops
    h, w, B = 37, 53, 19
    cases = R.op_cases(h, w)
    rng = random.Random(19)
    seqs = [[None if rng.random() < 0.2 else rng.choice(cases) for _ in range(3)] for _ in range(B)]
    seqs[0] = [None, None, None]
    seqs[1] = [("Equalize", None, None)] * 2 + [None]
    seqs[2] = [("SharpnessIncreasing", 1.9, None), None, ("SharpnessIncreasing", 1.9, None)]
    seqs[3] = [("Rotate", 30.0, BIC), ("ContrastIncreasing", 0.1, None), ("AutoContrast", None, None)]
    assert {c[0] for s in seqs for c in s if c} >= {"Equalize", "AutoContrast", "ContrastIncreasing", "Rotate"}
    kinds = R.images(h, w)
    host = np.stack([kinds[i % 5] if i % 3 else R.images(h, w, seed=i + 1)[0] for i in range(B)])
    fields = [R.fields(s, w, h) for s in seqs]
    op = torch.from_numpy(np.stack([f[0] for f in fields])).cuda()
    par = torch.from_numpy(np.stack([f[1] for f in fields])).cuda()
    src = torch.from_numpy(host).cuda()
    G = Guarded(torch)
    cur = src
    for slot in range(3):
        cur = _run_slot(ops, G, cur, op, par, slot)
    got = cur.cpu().numpy()
    G.check()
    assert np.array_equal(src.cpu().numpy(), host)
    for i, seq in enumerate(seqs):
        img = Image.fromarray(host[i])
        for case in seq:
            if case is not None:
                img = R.pillow_op(img, *case)
        assert np.array_equal(got[i], np.asarray(img)), (i, seq)


CHAINS = {"crop": {"RandomResizedCrop": 224, "RandomHorizontalFlip": None},
          "resize_crop": {"Resize": 240, "RandomResizedCrop": 224, "RandomHorizontalFlip": None}}
NORM = {"Mean": [0.485, 0.456, 0.406], "Std": [0.229, 0.224, 0.225]}


@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic", "random"])
@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("h,w", [(256, 256), (200, 333)])
def test_device_chain_equals_host_chain(h, w, chain, interpolation):
    from myrtle_vision.datasets.device_transforms import DevicePlan
    from myrtle_vision.datasets.transforms import build_transform
    cfg = dict(CHAINS[chain], Normalize=NORM, RandAugment={"prob": 1.0, "interpolation": interpolation})
    rng = np.random.default_rng(h + len(chain))
    imgs = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(8)]
    plan, host = DevicePlan(cfg), build_transform(cfg)
    seed = 1000 + h + 7 * len(chain) + len(interpolation)
    random.seed(seed)
    want = [host(i)[0] for i in imgs]
    random.seed(seed)
    packed, _ = DevicePlan.collate([(plan(i), 0) for i in imgs])
    assert (packed["ra_op"] > 0).all()                               # prob 1: no sample passes by skipping
    got, masks = plan.apply(packed, torch.device("cuda"))
    torch.cuda.synchronize()
    assert masks is None and got.dtype == torch.float32 and tuple(got.shape) == (8, 3, 224, 224)
    for i, t in enumerate(want):
        assert torch.equal(got[i].cpu(), t), (i, packed["ra_op"][i].tolist())


def test_without_the_key_apply_is_one_image_prepare():
    from myrtle_vision.datasets.device_transforms import DevicePlan
    from myrtle_vision.hip import ops
    cfg = dict(CHAINS["crop"], Normalize=NORM)
    rng = np.random.default_rng(4)
    imgs = [Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)) for _ in range(8)]
    plan = DevicePlan(cfg)
    random.seed(4)
    packed, _ = DevicePlan.collate([(plan(i), 0) for i in imgs])
    assert set(packed) == {"raw", "kh", "bh", "kv", "bv", "flip"} and packed["flip"].any()
    got, masks = plan.apply(packed, torch.device("cuda"))
    d = {k: v.cuda() for k, v in packed.items()}
    want = ops.image_prepare(d["raw"], d["kh"], d["bh"], d["kv"], d["bv"], d["flip"], plan.mean, plan.std)
    assert masks is None and torch.equal(got, want)
