"""RandAugment, host side: the config surface, the draw mapping, the worker's fields against what the host chain applied, the
rotate matrix, the packed batch, the shipped configs, the C ABI -- and csrc/randaug_math.h (the arithmetic the kernels inline)
compiled for the host and held to Pillow byte for byte.  No GPU needed; every comparison is exact."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import randaug_ref as R
from randaug_ref import BIC, BIL, ROOT

NORM = {"Mean": [0.485, 0.456, 0.406], "Std": [0.229, 0.224, 0.225]}


def _cfg(ra=None, **chain):
    cfg = dict(chain or {"RandomResizedCrop": 64, "RandomHorizontalFlip": None}, Normalize=NORM)
    if ra is not None:
        cfg["RandAugment"] = ra
    return cfg


def _pil(h, w, seed=0):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


# ---------------------------------------------------------------- config
@pytest.mark.parametrize("bad,word", [({"magnitud": 9}, "magnitud"), ({"magnitude": 11}, "magnitude"), ({"magnitude": -1}, "magnitude"),
                                      ({"magnitude": "9"}, "magnitude"), ({"magnitude_std": -0.5}, "magnitude_std"),
                                      ({"num_ops": 0}, "num_ops"), ({"num_ops": 2.0}, "num_ops"), ({"num_ops": True}, "num_ops"),
                                      ({"prob": 1.5}, "prob"), ({"prob": -0.1}, "prob"), ({"interpolation": "nearest"}, "interpolation"),
                                      ({"interpolation": 3}, "interpolation")])
def test_bad_config_raises_and_names_it_on_both_chains(bad, word):
    from myrtle_vision.datasets.device_transforms import DevicePlan
    from myrtle_vision.datasets.transforms import build_transform
    for build in (build_transform, DevicePlan):
        with pytest.raises(ValueError, match=word):
            build(_cfg(bad))


def test_defaults_and_fill_colour():
    from myrtle_vision.datasets.transforms import RandAugment, build_transform
    ra = build_transform(_cfg({})).ops[-2]
    assert isinstance(ra, RandAugment)
    assert (ra.magnitude, ra.magnitude_std, ra.num_ops, ra.prob, ra.interpolation) == (9.0, 0.5, 2, 0.5, "bicubic")
    assert ra.fill == (124, 116, 104)
    assert RandAugment().fill == (128, 128, 128) and RandAugment(None, [1.0, 0.999, 0.0]).fill == (255, 255, 0)


def test_a_mask_raises_on_both_chains():
    from myrtle_vision.datasets.device_transforms import DevicePlan
    from myrtle_vision.datasets.transforms import build_transform
    img, mask = _pil(80, 80), Image.fromarray(np.ones((80, 80), np.uint8))
    for chain in (build_transform(_cfg({})), DevicePlan(_cfg({}))):
        with pytest.raises(ValueError, match="classification"):
            chain(img, mask)


def test_without_the_key_the_chain_is_what_it_was():
    from myrtle_vision.datasets import transforms as T
    full = {"Resize": 96, "RandomResizedCrop": 64, "CenterCrop": 48, "RandomHorizontalFlip": None, "Normalize": NORM}
    names = lambda cfg: [type(o).__name__ for o in T.build_transform(cfg).ops]
    assert names(full) == ["Resize", "RandomResizedCrop", "CenterCrop", "RandomHorizontalFlip", "ToTensorNormalize"]
    assert names({"Resize": 96}) == ["Resize", "ToTensorNormalize"]
    assert names(dict(full, RandAugment={})) == ["Resize", "RandomResizedCrop", "CenterCrop", "RandomHorizontalFlip", "RandAugment",
                                                 "ToTensorNormalize"]


# ---------------------------------------------------------------- draw mapping
def _all_arguments(magnitude, seeds=400, **kw):
    """{op name: set of arguments} over many draws at a fixed magnitude, 100 x 50 image."""
    from myrtle_vision.datasets.transforms import RandAugment
    ra = RandAugment(dict({"magnitude": magnitude, "magnitude_std": 0, "prob": 1.0, "num_ops": 3}, **kw))
    seen = {}
    for seed in range(seeds):
        random.seed(seed)
        for name, arg, _ in ra.draw(100, 50):
            seen.setdefault(name, set()).add(arg)
    assert set(seen) == set(R.OPS)
    return seen


def test_draw_mapping_at_the_limits():
    lo, hi = _all_arguments(0), _all_arguments(10)
    for name in ("AutoContrast", "Equalize", "Invert"):
        assert lo[name] == hi[name] == {None}
    assert lo["Rotate"] == {0.0} and hi["Rotate"] == {30.0, -30.0}
    assert lo["ShearX"] == lo["ShearY"] == {0.0} and hi["ShearX"] == hi["ShearY"] == {0.3, -0.3}
    assert lo["TranslateXRel"] == lo["TranslateYRel"] == {0.0}
    assert hi["TranslateXRel"] == {45.0, -45.0} and hi["TranslateYRel"] == {22.5, -22.5}
    assert lo["PosterizeIncreasing"] == {4} and hi["PosterizeIncreasing"] == {0}
    assert lo["SolarizeIncreasing"] == {256} and hi["SolarizeIncreasing"] == {0}
    assert lo["SolarizeAdd"] == {0} and hi["SolarizeAdd"] == {110}
    for name in R.ENHANCE:
        assert lo[name] == {1.0} and hi[name] == {0.1, 1.9}          # 1 - 0.9 is below 0.1 in binary: the floor holds


def test_gaussian_magnitudes_are_clamped():
    from myrtle_vision.datasets.transforms import RandAugment
    ra = RandAugment({"magnitude": 9, "magnitude_std": 40.0, "prob": 1.0, "num_ops": 4})
    rot, fac, bits = set(), set(), set()
    for seed in range(300):
        random.seed(seed)
        for name, arg, _ in ra.draw(64, 64):
            if name == "Rotate":
                rot.add(arg)
            elif name in R.ENHANCE:
                fac.add(arg)
            elif name == "PosterizeIncreasing":
                bits.add(arg)
    assert {30.0, -30.0} <= rot and 0.0 in {abs(r) for r in rot} and max(abs(r) for r in rot) == 30.0
    assert min(fac) == 0.1 and max(fac) == 1.9 and bits <= {0, 1, 2, 3, 4} and {0, 4} <= bits


def test_prob_zero_skips_every_slot_after_the_op_draws():
    from myrtle_vision.datasets.transforms import RandAugment
    random.seed(5)
    assert RandAugment({"prob": 0.0, "num_ops": 3}).draw(8, 8) == [None, None, None]
    state = random.getstate()
    random.seed(5)
    for _ in range(3):
        random.randrange(15)
    for _ in range(3):
        random.random()
    assert random.getstate() == state                               # 3 op draws + 3 probability draws, nothing else


# ---------------------------------------------------------------- the worker draws what the host chain applies
@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic", "random"])
def test_device_plan_fields_equal_what_the_host_chain_applied(interpolation):
    from myrtle_vision.datasets.device_transforms import DevicePlan
    from myrtle_vision.datasets.transforms import RANDAUG_OPS, affine_coefficients, build_transform
    ra = {"interpolation": interpolation, "num_ops": 3, "prob": 0.7}
    cfg, bare = _cfg(ra), _cfg(None)
    host, plan, plan_bare = build_transform(cfg), DevicePlan(cfg), DevicePlan(bare)
    img = _pil(80, 96)
    skipped = 0
    for seed in range(200):
        random.seed(seed)
        host(img)
        applied = host.ops[-2].applied
        random.seed(seed)
        s = plan(img)
        random.seed(seed)
        s0 = plan_bare(img)
        # crop box and flip: drawn first, so the key does not move them; the flip is folded into the horizontal tables
        assert s["flip"] == 0 and torch.equal(s["kv"], s0["kv"]) and torch.equal(s["bv"], s0["bv"])
        kh0, bh0 = (s0["kh"].flip(0), s0["bh"].flip(0)) if s0["flip"] else (s0["kh"], s0["bh"])
        assert torch.equal(s["kh"], kh0) and torch.equal(s["bh"], bh0)
        op, par = s["ra_op"].numpy(), s["ra_par"].numpy()
        assert op.dtype == np.int32 and op.shape == (3,) and par.dtype == np.float64 and par.shape == (3, 8)
        for i, slot in enumerate(applied):
            if slot is None:
                assert op[i] == 0 and not par[i].any()
                skipped += 1
                continue
            name, arg, resample = slot
            assert RANDAUG_OPS[op[i] - 1] == name == R.OPS[op[i] - 1]
            if name in R.GEOMETRIC:
                assert tuple(par[i, :6]) == tuple(float(v) for v in affine_coefficients(name, arg, 64, 64))
                assert par[i, 6] == (1.0 if resample == BIC else 0.0) and resample in (BIL, BIC)
                if interpolation != "random":
                    assert resample == {"bilinear": BIL, "bicubic": BIC}[interpolation]
            else:
                assert par[i, 0] == (0.0 if arg is None else arg) and not par[i, 1:].any()
    assert skipped > 0


# ---------------------------------------------------------------- Rotate is an affine
@pytest.mark.parametrize("h,w", [(37, 53), (224, 224)])
@pytest.mark.parametrize("resample", [BIL, BIC])
def test_rotate_matrix_reproduces_image_rotate(h, w, resample):
    from myrtle_vision.datasets.transforms import rotate_matrix
    img = _pil(h, w, 3)
    rng = random.Random(h)
    angles = [0.0, 30.0, -30.0, 90.0, -0.0, 29.999, 1e-9] + [rng.uniform(-30, 30) for _ in range(13)]
    assert len(angles) == 20
    for deg in angles:
        want = img.rotate(deg, resample, fillcolor=R.FILL)
        got = img.transform((w, h), Image.Transform.AFFINE, rotate_matrix(deg, w, h), resample, fillcolor=R.FILL)
        assert np.array_equal(np.asarray(got), np.asarray(want)), deg


# ---------------------------------------------------------------- the packed batch
def test_packed_batch_keys():
    from myrtle_vision.datasets.device_transforms import DevicePlan
    today = {"raw", "kh", "bh", "kv", "bv", "flip"}
    imgs = [_pil(80, 96, i) for i in range(4)]
    for chain, extra in (({"RandomResizedCrop": 64, "RandomHorizontalFlip": None}, set()),
                         ({"Resize": 72, "RandomResizedCrop": 64, "RandomHorizontalFlip": None}, {"kh1", "bh1", "kv1", "bv1"})):
        def sample(plan, k):                                         # seeded per image: RandAugment's draws follow the flip's
            random.seed(100 + k)
            return plan(imgs[k])
        plan = DevicePlan(_cfg(None, **chain))
        packed, labels = DevicePlan.collate([(sample(plan, k), 1) for k in range(4)])
        assert set(packed) == today | extra
        plan = DevicePlan(_cfg({"num_ops": 3}, **chain))
        with_key, _ = DevicePlan.collate([(sample(plan, k), 1) for k in range(4)])
        assert set(with_key) == today | extra | {"ra_op", "ra_par"}
        assert with_key["ra_op"].dtype == torch.int32 and tuple(with_key["ra_op"].shape) == (4, 3)
        assert with_key["ra_par"].dtype == torch.float64 and tuple(with_key["ra_par"].shape) == (4, 3, 8)
        assert with_key["flip"].dtype == torch.uint8 and not with_key["flip"].any() and packed["flip"].any()
        for b in range(4):                                           # same crop; a flipped sample's rows are reversed
            rev = (lambda t: t.flip(0)) if packed["flip"][b] else (lambda t: t)
            assert torch.equal(with_key["kh"][b], rev(packed["kh"][b])) and torch.equal(with_key["bh"][b], rev(packed["bh"][b]))
            assert torch.equal(with_key["kv"][b], packed["kv"][b]) and torch.equal(with_key["raw"][b], packed["raw"][b])


def test_plan_goes_to_a_worker_without_its_device_tables():
    import pickle
    from myrtle_vision.datasets.device_transforms import DevicePlan
    plan = DevicePlan(_cfg({"num_ops": 1}))
    plan._identity["key"] = object()                                 # stands for the device-resident copying tables of ``apply``
    clone = pickle.loads(pickle.dumps(plan))
    assert clone._identity == {} and clone.randaug.num_ops == 1 and "key" in plan._identity
    random.seed(3)
    a = plan(_pil(80, 96))
    random.seed(3)
    b = clone(_pil(80, 96))
    assert all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


# ---------------------------------------------------------------- shipped configs
def test_shipped_configs_build_both_chains():
    from myrtle_vision.datasets.device_transforms import DevicePlan
    from myrtle_vision.datasets.transforms import RandAugment, build_transform
    base = json.load(open(os.path.join(ROOT, "classification", "data_configs", "data_config.json")))
    data = json.load(open(os.path.join(ROOT, "classification", "data_configs", "data_config_randaug.json")))
    assert data["transform_ops_train"].pop("RandAugment") == {"magnitude": 9, "magnitude_std": 0.5, "num_ops": 2, "prob": 0.5,
                                                               "interpolation": "bicubic"}
    assert data == base                                              # data_config.json plus the key in transform_ops_train only
    data = json.load(open(os.path.join(ROOT, "classification", "data_configs", "data_config_randaug.json")))
    for section, has in (("transform_ops_train", True), ("transform_ops_val", False)):
        host, plan = build_transform(data[section]), DevicePlan(data[section])
        assert any(isinstance(o, RandAugment) for o in host.ops) == has and (plan.randaug is not None) == has
    train = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_base_mixup_re_ra.json")))
    parent = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_base_mixup_re.json")))
    assert train.pop("data_config_path").endswith("data_config_randaug.json") and parent.pop("data_config_path")
    assert train == parent


# ---------------------------------------------------------------- C ABI
def test_c_abi():
    from myrtle_vision.hip import lib
    assert lib.SIGNATURES["mv_randaug_stats"] == ("pp" "ii" "pp" "iii" "p", ctypes.c_int)
    assert lib.SIGNATURES["mv_randaug_apply"] == ("pppp" "ii" "pp" "iii" "iii" "p", ctypes.c_int)
    header = open(os.path.join(ROOT, "include", "myrtle_vision_hip.h")).read()
    assert "int mv_randaug_stats(" in header and "int mv_randaug_apply(" in header
    h = lib.lib()
    MV_ERR_SHAPE, MV_ERR_ALIGN = -1, -2
    assert h.mv_randaug_stats(None, None, 2, 0, None, None, 0, 8, 8, None) == 0            # B == 0: nothing looked at
    assert h.mv_randaug_stats(None, None, 2, 2, None, None, 4, 8, 8, None) == MV_ERR_SHAPE  # slot outside [0, num_ops)
    assert h.mv_randaug_stats(None, None, 2, 0, None, None, 4, 8, 8, None) == MV_ERR_ALIGN  # null arrays
    assert h.mv_randaug_apply(None, None, None, None, 2, 0, None, None, 0, 0, 0, 4, 0, 8, None) == MV_ERR_SHAPE
    assert h.mv_randaug_apply(None, None, None, None, 2, 0, None, None, 0, 0, 0, 4, 8, 8, None) == MV_ERR_ALIGN


# ---------------------------------------------------------------- the kernels' arithmetic, compiled for the host, against Pillow
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return R.host_library(tmp_path_factory.mktemp("randaug_host"))


def test_host_chain_ops_are_the_direct_pillow_calls():
    from myrtle_vision.datasets.transforms import RandAugment
    ra = RandAugment(None, NORM["Mean"])
    for a in R.images(37, 53):
        img = Image.fromarray(a)
        for name, arg, resample in R.op_cases(37, 53):
            assert np.array_equal(np.asarray(ra.apply_op(img, name, arg, resample)), np.asarray(R.pillow_op(img, name, arg, resample)))


@pytest.mark.parametrize("h,w", R.SIZES[:4])
def test_kernel_arithmetic_on_the_host_equals_pillow(host, h, w):
    for k, a in enumerate(R.images(h, w)):
        img = Image.fromarray(a)
        for name, arg, resample in R.op_cases(h, w):
            want = np.asarray(R.pillow_op(img, name, arg, resample))
            assert np.array_equal(R.host_op(host, a, name, arg, resample), want), (k, name, arg, resample)


def test_kernel_arithmetic_on_the_host_random_parameters(host):
    rng = random.Random(11)
    a = R.images(37, 53)[0]
    img = Image.fromarray(a)
    for _ in range(40):
        resample = rng.choice((BIL, BIC))
        for name, arg in (("Rotate", rng.uniform(-30, 30)), ("ShearX", rng.uniform(-0.3, 0.3)), ("ShearY", rng.uniform(-0.3, 0.3)),
                          ("TranslateXRel", rng.uniform(-0.45, 0.45) * 53), ("TranslateYRel", rng.uniform(-0.45, 0.45) * 37)):
            assert np.array_equal(R.host_op(host, a, name, arg, resample), np.asarray(R.pillow_op(img, name, arg, resample))), (name, arg)
        for name in R.ENHANCE:
            f = rng.uniform(0.05, 1.95)
            assert np.array_equal(R.host_op(host, a, name, f, None), np.asarray(R.pillow_op(img, name, f))), (name, f)


def test_autocontrast_table_at_every_range_on_the_host(host):
    for a in R.autocontrast_images():
        want = np.asarray(R.pillow_op(Image.fromarray(a), "AutoContrast"))
        assert np.array_equal(R.host_op(host, a, "AutoContrast", None, None), want)
