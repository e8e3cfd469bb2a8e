"""GPU: the fused segmentation tail with a recipe (mv_seg_loss_fwd / _bwd: class weights, label smoothing, Dice) against the torch
composition of tests/seg_loss_ref.py in fp64, at the smallest shapes at which the kernels can go wrong, with guard zones round every
buffer they write; then one case at the workload's grid, and the model-level interface.

Exact: pred (the fp64 arg-max; every input keeps a margin > 1e-3, asserted), pred / lse against mv_seg_ce_fwd bit for bit, areas,
stats[1..3], the zero columns of a padded gradient, two runs against each other, a power-of-two grad_scale.
Floating point (stats[0, 4, 5, 6], coef, dsmall): the project's standing rule for a kernel against a torch composition -- 8 x the error
of the SAME formulas evaluated by torch in fp32 against fp64, measured per case in this run, never below 4 fp32 ulps of the value's
magnitude (for a tensor: largest elementwise error against 8 x torch's largest elementwise error, floor at the largest magnitude).
bf16 dsmall: that bar plus one bf16 rounding of the element.  With MV_SEG_LOSS_PARITY_OUT set, every measured error and its bar is
written to that file (profiles/seg_loss_parity.txt is such a run)."""
import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402
import seg_loss_ref as ref  # noqa: E402

OK, SHAPE, UNSUPPORTED = 0, -1, -4
GUARD = 64                                                   # elements on each side
SENTINEL = {torch.float32: 12345.0, torch.bfloat16: 12345.0, torch.uint8: 0xA5, torch.int64: -7777777}
PARITY = []                                                  # (case, quantity, error, bar, torch's fp32 error)


@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    path = os.environ.get("MV_SEG_LOSS_PARITY_OUT")
    if path and PARITY:
        with open(path, "w") as f:
            f.write("# mv_seg_loss_* against tests/seg_loss_ref.py in fp64 (tests/test_seg_loss_gpu.py).  error = kernel - fp64; bar = max(8 x\n"
                    "# torch32, 4 fp32 ulps of the magnitude); torch32 = the same torch composition in fp32 against fp64, in the same run.\n"
                    "# Tensors: largest elementwise error.  Model rows: relative L2 per tensor.\n")
            f.write(f"{'case':<52} {'quantity':<44} {'error':>10} {'bar':>10} {'torch32':>10}\n")
            for case, q, e, bar, e32 in PARITY:
                f.write(f"{case:<52} {q:<44} {e:>10.3e} {bar:>10.3e} {e32:>10.3e}\n")


def under(case, quantity, err, bar, err32):
    PARITY.append((case, quantity, err, bar, err32))
    print(f"{case} {quantity}: error {err:.3e} bar {bar:.3e} (torch fp32 {err32:.3e})")
    return err <= bar


class Guarded:
    """A device buffer with GUARD sentinel elements on each side of the part the kernel may write."""

    def __init__(self, shape, dtype):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.dtype = dtype

    def intact(self):
        s = SENTINEL[self.dtype]
        return bool((self.buf[:GUARD] == s).all()) and bool((self.buf[-GUARD:] == s).all())

    def untouched(self):
        return bool((self.buf == SENTINEL[self.dtype]).all())


def run_kernels(small, y, wts, eps, lam, s, dims, *, grad_dtype=torch.float32, ld=None, grad_scale=1.0, backward=True):
    """mv_seg_loss_fwd (+ _bwd) on guarded buffers -> dict of the outputs (views into the guarded buffers) after checking every guard."""
    from myrtle_vision.hip.lib import lib
    from myrtle_vision.hip.ops import _DT, _p, _s
    B, C, h, w, H, W = dims
    ld = C if ld is None else ld
    small, y = small.cuda().contiguous(), y.cuda().contiguous()
    cw = None if wts is None else wts.float().cuda().contiguous()
    g = dict(lse=Guarded((B, H, W), torch.float32), pred=Guarded((B, H, W), torch.uint8), stats=Guarded((8,), torch.float32),
             coef=Guarded((2, C), torch.float32), areas=Guarded((3, C), torch.int64),
             partials=Guarded((max(lib().mv_seg_loss_partials(B, C, H, W), 4),), torch.float32),
             dsmall=Guarded((B * h * w, ld), grad_dtype))
    rc = lib().mv_seg_loss_fwd(_p(small), _p(y), _p(cw), eps, lam, s, _p(g["lse"].t), _p(g["pred"].t), _p(g["partials"].t),
                               _p(g["stats"].t), _p(g["coef"].t), _p(g["areas"].t), B, C, h, w, H, W, _s())
    assert rc == OK, rc
    if backward:
        rc = lib().mv_seg_loss_bwd(_p(small), _p(y), _p(cw), eps, lam, _p(g["lse"].t), _p(g["stats"].t), _p(g["coef"].t),
                                   _p(g["dsmall"].t), _DT[grad_dtype], ld, grad_scale, B, C, h, w, H, W, _s())
        assert rc == OK, rc
    torch.cuda.synchronize()
    for name, buf in g.items():
        assert buf.intact(), f"{name}: a guard zone was written"
    return {k: v.t for k, v in g.items()}


@functools.lru_cache(maxsize=None)
def case_data(shape, labeling, option):
    """Inputs and both references (fp64, and torch's fp32 for the bar) of one case; computed once, never modified."""
    B, C, h, w, H, W, seed = shape
    use_w, eps, lam, s = ref.OPTIONS[option]
    small = ref.make_small(B, C, h, w, seed)
    y, wts = ref.make_labels(B, C, H, W, seed, labeling)
    wts = wts if use_w else None
    dims = (B, C, h, w, H, W)
    r64 = ref.reference(small, y, dims, wts, eps, lam, s, torch.float64)
    r32 = ref.reference(small, y, dims, wts, eps, lam, s, torch.float32)
    return small, y, wts, dims, (eps, lam, s), r64, r32


def check_floats(case, out, r64, r32):
    """Every floating-point output of one case against its bar; all of them are measured before the first one fails the test."""
    over = []
    for i, name in ((0, "loss"), (4, "ce"), (5, "dice"), (6, "W")):
        got, want, w32 = float(out["stats"][i]), r64["stats"][i], r32["stats"][i]
        if math.isnan(want):
            assert math.isnan(got), (name, got)
            continue
        assert math.isfinite(got), (name, got)
        if not under(case, name, abs(got - want), ref.scalar_bar(w32, want), abs(w32 - want)):
            over.append(name)
    for name in ("coef", "dsmall"):
        got = out[name].double().cpu()
        e32 = float((r32[name].double() - r64[name]).abs().max())
        if not under(case, name, float((got - r64[name]).abs().max()), ref.tensor_bar(r32[name], r64[name]), e32):
            over.append(name)
    assert not over, over


# ================================================================== the kernels at the smallest shapes
@pytest.mark.parametrize("option", list(ref.OPTIONS))
@pytest.mark.parametrize("labeling", ref.LABELINGS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.SHAPE_IDS)
def test_kernels_against_fp64(ops, shape, labeling, option):
    small, y, wts, dims, (eps, lam, s), r64, r32 = case_data(shape, labeling, option)
    B, C, h, w, H, W = dims
    case = f"{ref.SHAPE_IDS[ref.SHAPES.index(shape)]}/{labeling}/{option}"
    assert r64["margin"] > 1e-3                               # no pixel is excluded from the arg-max comparison
    out = run_kernels(small, y, wts, eps, lam, s, dims)
    # exact outputs
    assert torch.equal(out["pred"].cpu().long(), r64["pred"])
    assert torch.equal(out["areas"].cpu(), r64["areas"])
    st = out["stats"].cpu()
    assert float(st[1]) == float(torch.tensor(r64["stats"][1], dtype=torch.float32))
    assert float(st[2]) == r64["stats"][2] and float(st[3]) == r64["stats"][3] and float(st[7]) == 0.0
    if ops.seg_ce_supported(C, h, w, W):                      # the plain tail on the same inputs: the same lse and arg-max, bit for bit
        stats_p, lse_p, pred_p, _ = ops.seg_ce_fwd(small.cuda(), y.cuda(), B, C, h, w, H, W)
        assert torch.equal(out["lse"], lse_p) and torch.equal(out["pred"], pred_p)
        # (its accuracy is hits x fp32(1 / pixels), an ulp off the correctly rounded quotient that stats[1] holds here)
        assert float(st[2]) == float(stats_p[2]) and float(st[3]) == float(stats_p[3])
    assert float((out["lse"].double().cpu() - r64["lse"]).abs().max()) <= max(
        8.0 * float((r32["lse"].double() - r64["lse"]).abs().max()), 4.0 * ref.ulp32(float(r64["lse"].abs().max())))
    # the NaN rules and the zero gradient that goes with a missing denominator
    if labeling in ("all_ignored", "out_of_range") or (labeling == "all_zero_weight" and wts is not None):
        assert math.isnan(float(st[0])) and math.isnan(float(st[4]))
    else:
        assert math.isfinite(float(st[0]))
    if labeling == "all_ignored" or (labeling == "all_zero_weight" and wts is not None):
        assert float(st[6]) == 0.0 and not out["dsmall"].any()
    if labeling == "all_ignored":
        assert float(st[5]) == 0.0
    if lam == 0.0:
        assert float(st[5]) == 0.0 and not out["coef"].any()
    check_floats(case, out, r64, r32)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.SHAPE_IDS)
def test_reproducible_scaled_and_padded_bf16(shape):
    """Two runs are bitwise equal; a power-of-two grad_scale scales dsmall exactly; the bf16 layout [M, ld] holds the same gradient
    to the fp32 bar plus one bf16 rounding of the element, with columns [C, ld) exactly zero."""
    small, y, wts, dims, (eps, lam, s), r64, r32 = case_data(shape, "ignored", "all")
    B, C, h, w, H, W = dims
    case = f"{ref.SHAPE_IDS[ref.SHAPES.index(shape)]}/ignored/all"
    one = run_kernels(small, y, wts, eps, lam, s, dims)
    two = run_kernels(small, y, wts, eps, lam, s, dims)
    for k in ("lse", "pred", "coef", "areas", "dsmall"):
        assert torch.equal(one[k], two[k]), k
    assert torch.equal(one["stats"].view(torch.int32), two["stats"].view(torch.int32))
    scaled = run_kernels(small, y, wts, eps, lam, s, dims, grad_scale=0.25)
    assert torch.equal(scaled["dsmall"], one["dsmall"] * 0.25)
    ld = (C + 7) // 8 * 8 + 8                                 # at least eight columns of padding
    pad = run_kernels(small, y, wts, eps, lam, s, dims, grad_dtype=torch.bfloat16, ld=ld)
    assert not pad["dsmall"][:, C:].any()
    got, want = pad["dsmall"][:, :C].double().cpu(), r64["dsmall"]
    bar = ref.tensor_bar(r32["dsmall"], want) + want.abs() * 2.0 ** -8          # one bf16 rounding: half an ulp of 2^-7
    err = (got - want).abs()
    PARITY.append((case, "dsmall bf16", float(err.max()), float(bar.max()), float((r32["dsmall"].double() - want).abs().max())))
    assert bool((err <= bar).all()), float((err - bar).max())


def test_bad_arguments_return_their_codes_without_a_launch():
    from myrtle_vision.hip.lib import lib
    from myrtle_vision.hip.ops import _p, _s
    B, C, h, w, H, W = 2, 5, 2, 2, 4, 4
    small = torch.randn(B * h * w, 40, device="cuda")
    y = torch.zeros(B, H, W, dtype=torch.int64, device="cuda")
    bufs = dict(lse=Guarded((B, H, W), torch.float32), pred=Guarded((B, H, W), torch.uint8), stats=Guarded((8,), torch.float32),
                coef=Guarded((2, 40), torch.float32), areas=Guarded((3, 40), torch.int64), partials=Guarded((4096,), torch.float32),
                dsmall=Guarded((B * h * w, 40), torch.float32))

    def fwd(C=C, eps=0.0, lam=0.0, s=1.0, B=B, H=H):
        return lib().mv_seg_loss_fwd(_p(small), _p(y), None, eps, lam, s, _p(bufs["lse"].t), _p(bufs["pred"].t), _p(bufs["partials"].t),
                                     _p(bufs["stats"].t), _p(bufs["coef"].t), _p(bufs["areas"].t), B, C, h, w, H, W, _s())

    def bwd(C=C, eps=0.0, lam=0.0, elem=0, ld=40, B=B):
        return lib().mv_seg_loss_bwd(_p(small), _p(y), None, eps, lam, _p(bufs["lse"].t), _p(bufs["stats"].t), _p(bufs["coef"].t),
                                     _p(bufs["dsmall"].t), elem, ld, 1.0, B, C, h, w, H, W, _s())

    assert fwd(C=33) == UNSUPPORTED and bwd(C=33) == UNSUPPORTED
    assert fwd(eps=-0.1) == UNSUPPORTED and fwd(eps=1.0) == UNSUPPORTED and fwd(lam=-1.0) == UNSUPPORTED
    assert fwd(lam=0.5, s=0.0) == UNSUPPORTED and fwd(lam=0.5, s=-2.0) == UNSUPPORTED
    assert bwd(eps=1.0) == UNSUPPORTED and bwd(lam=-1.0) == UNSUPPORTED and bwd(elem=2) == UNSUPPORTED
    assert fwd(B=65536) == SHAPE and fwd(H=0) == SHAPE and bwd(ld=4) == SHAPE and bwd(B=65536) == SHAPE
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert b.untouched(), f"{name} was written"


def test_empty_batch_clears_stats_and_areas():
    from myrtle_vision.hip.lib import lib
    from myrtle_vision.hip.ops import _p, _s
    C = 17
    stats, areas = Guarded((8,), torch.float32), Guarded((3, C), torch.int64)
    other = Guarded((64,), torch.float32)
    p = _p(other.t)
    assert lib().mv_seg_loss_fwd(p, p, None, 0.1, 0.5, 1.0, p, p, p, _p(stats.t), p, _p(areas.t), 0, C, 14, 14, 224, 224, _s()) == OK
    torch.cuda.synchronize()
    assert not stats.t.any() and not areas.t.any() and stats.intact() and areas.intact() and other.untouched()
    stats.t.fill_(3.0)
    assert lib().mv_seg_loss_fwd(p, p, None, 0.0, 0.0, 1.0, p, p, p, _p(stats.t), p, None, 0, C, 14, 14, 224, 224, _s()) == OK     # no areas
    assert lib().mv_seg_loss_bwd(p, p, None, 0.0, 0.0, p, p, p, p, 0, C, 1.0, 0, C, 14, 14, 224, 224, _s()) == OK
    torch.cuda.synchronize()
    assert not stats.t.any() and stats.intact() and other.untouched()


# ================================================================== the workload's grid
def test_workload_grid(ops):
    """B = 2, C = 17, 14x14 -> 224x224: 100 352 pixels, where no arg-max margin can be guaranteed, so nothing is compared with the
    fp64 arg-max: pred / lse bit for bit against mv_seg_ce_fwd, the areas against bincounts of THAT pred, the float outputs under the bar."""
    small, y, wts, dims, (eps, lam, s), r64, r32 = case_data(ref.WORKLOAD_SHAPE, "ignored", "all")
    B, C, h, w, H, W = dims
    out = run_kernels(small, y, wts, eps, lam, s, dims)
    stats_p, lse_p, pred_p, _ = ops.seg_ce_fwd(small.cuda(), y.cuda(), B, C, h, w, H, W)
    assert torch.equal(out["lse"], lse_p) and torch.equal(out["pred"], pred_p)
    assert torch.equal(out["areas"].cpu(), ref.areas(pred_p.cpu(), y, C))
    st = out["stats"].cpu()
    hits = int((pred_p.cpu().long() == y).sum())
    assert float(st[1]) == float(torch.tensor(hits / y.numel(), dtype=torch.float32))
    assert float(st[2]) == float(stats_p[2]) and float(st[3]) == 0.0
    check_floats("workload-B2-C17-14x14-to-224x224/ignored/all", out, r64, r32)


# ================================================================== the model-level interface
def _micro(precision):
    from myrtle_vision.models.vit import ViT
    # image_size 80, not 64: the constructor refuses the 16 patches of 64 / 16 (reference vit.py:14, MIN_NUM_PATCHES)
    torch.manual_seed(11)
    vit = ViT(decoder="segmentation", image_size=80, patch_size=16, num_classes=5, dim=64, depth=1, heads=1, mlp_dim=64,
              precision=precision).cuda()
    vit.train()
    g = torch.Generator().manual_seed(12)
    img = torch.randn(2, 3, 80, 80, generator=g).cuda()
    labels = torch.randint(0, 5, (2, 80, 80), generator=g)
    labels[0, :9, :] = ref.IGNORE
    return vit, img, labels


def _grads(vit):
    out = {n: p.grad.detach().double().cpu().clone() for n, p in vit.named_parameters() if p.grad is not None}
    for p in vit.parameters():
        p.grad = None
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_loss_and_parameter_gradients(precision):
    """``segmentation_loss(img, labels, loss=spec)`` against the same model's ``vit(img)`` logits put through the fp64 reference with
    autograd: the loss and every parameter gradient (relative L2 per tensor) under 8 x what the fp32 torch composition of the tail
    gives on those logits."""
    from myrtle_vision.hip.functional import SegLoss
    vit, img, labels = _micro(precision)
    C = 5
    wts = torch.tensor([0.5, 1.25, 0.0, 2.0, 0.8])
    spec = SegLoss(wts.tolist(), 0.1, 0.5, 1.0)
    loss, acc, pred, areas = vit.segmentation_loss(img, labels.cuda(), loss=spec, return_areas=True)
    loss.backward()
    got = _grads(vit)
    tail = {}
    for dtype in (torch.float64, torch.float32):
        logits = vit(img)
        t = ref.terms(logits.to(dtype), labels.cuda(), wts.cuda(), ref.f32(0.1), ref.f32(0.5), 1.0)
        t["loss"].backward()
        tail[dtype] = (float(t["loss"].detach()), _grads(vit), logits.detach())
    (l64, g64, logits), (l32, g32, _) = tail[torch.float64], tail[torch.float32]
    case = f"model-{precision}"
    assert under(case, "loss", abs(float(loss.detach()) - l64), ref.scalar_bar(l32, l64), abs(l32 - l64))
    assert set(got) == set(g64)
    for name in sorted(g64):
        n64 = float(g64[name].norm())
        e = float((got[name] - g64[name]).norm()) / max(n64, 1e-300)
        e32 = float((g32[name] - g64[name]).norm()) / max(n64, 1e-300)
        assert under(case, name, e, max(8.0 * e32, 4.0 * 2.0 ** -24), e32), name
    want_pred = logits.argmax(1)
    assert float((pred.long() != want_pred).float().mean()) < 1e-3          # the tail's own interpolation: ties within fp32 rounding only
    assert torch.equal(areas.cpu(), ref.areas(pred.cpu(), labels, C))
    assert float(acc) == float((pred.cpu().long() == labels).float().mean())


def test_engine_trains_with_the_recipe_and_prints_the_training_miou(tmp_path, capsys, monkeypatch):
    """``train_config["seg_loss"]`` through ``train_worker``: every training step goes through ``segmentation_loss(..., loss=spec,
    return_areas=True)``, validation keeps the plain call, and the epoch line carries the mIoU of the areas -- the value ``add_img``
    gives on the same predictions."""
    import copy
    import json
    from myrtle_vision.datasets.synthetic import make_dlrsd
    from myrtle_vision.engine import train_worker
    from myrtle_vision.hip.functional import SegLoss
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.miou import MIoU
    cfg = json.load(open(os.path.join(ROOT, "segmentation", "train_configs", "seg_tiny.json")))
    data = json.load(open(os.path.join(ROOT, "segmentation", "data_configs", "data_config.json")))
    data["dataset_path"] = make_dlrsd(str(tmp_path / "DLRSD_dataset"), count=48)
    json.dump(data, open(str(tmp_path / "data_config.json"), "w"))
    cfg["data_config_path"] = str(tmp_path / "data_config.json")
    C = data["number_of_classes"]
    cfg["train_config"].update(output_directory=str(tmp_path / "ckpt"), epochs=1, local_batch_size=8, global_batch_size=8,
                               iters_per_checkpoint=1000, iters_per_val=1000, distributed=False, pretrained_backbone=None,
                               tensorboard_dir=str(tmp_path / "runs"),
                               seg_loss={"class_weights": [1.0 + 0.1 * c for c in range(C)], "label_smoothing": 0.1,
                                         "dice_weight": 0.5, "dice_smooth": 1.0})
    cfg["vit_config"]["depth"] = 2
    calls, inner = [], ViT.segmentation_loss

    def recording(self, img, labels, loss=None, return_areas=False):
        out = inner(self, img, labels, loss=loss, return_areas=return_areas)
        calls.append((self.training, loss, return_areas, out[2].clone(), labels.clone()))
        return out

    monkeypatch.setattr(ViT, "segmentation_loss", recording)
    iters = train_worker(0, 1, copy.deepcopy(cfg), "segmentation")
    out = capsys.readouterr().out
    train = [c for c in calls if c[0]]
    assert iters >= 2 and len(train) == iters and "nan" not in out.lower()
    assert all(type(c[1]) is SegLoss and c[2] for c in train) and train[0][1].dice_weight == 0.5 and len(train[0][1].class_weights) == C
    assert all(c[1] is None and not c[2] for c in calls if not c[0])            # validation: the plain criterion
    want = MIoU(C, "cuda")
    for _, _, _, pred, labels in train:
        want.add_img(pred, labels)
    epoch = [l for l in out.splitlines() if l.startswith("Epoch")]
    assert len(epoch) == 1 and f"train_miou: {want.get_miou():.4f}" in epoch[0], epoch


def test_default_call_is_the_plain_tail_bit_for_bit():
    """``segmentation_loss(img, labels)`` returns what it returned before: the 3-tuple of ``seg_head_loss``'s plain path, compared in
    the same run; ``return_areas=True`` alone adds the areas of that same arg-max."""
    from myrtle_vision.hip import functional as F
    vit, img, labels = _micro("fp32")
    labels = labels.cuda()
    out = vit.segmentation_loss(img, labels)
    assert len(out) == 3
    with torch.no_grad():
        x = vit._backbone(img)
    d = vit.decoder
    plain = F.seg_head_loss(x.float(), d.norm.weight, d.norm.bias, d.linear.weight, d.linear.bias, labels, d.image_size_in_patches,
                            d.image_size, d.norm.precision)
    assert len(plain) == 3
    assert torch.equal(out[0].detach().view(1).view(torch.int32), plain[0].detach().view(1).view(torch.int32))
    assert torch.equal(out[1], plain[1]) and torch.equal(out[2], plain[2])
    with torch.no_grad():
        four = vit.segmentation_loss(img, labels, return_areas=True)
    assert len(four) == 4 and torch.equal(four[2], out[2]) and torch.equal(four[3].cpu(), ref.areas(out[2].cpu(), labels.cpu(), 5))
