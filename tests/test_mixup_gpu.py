"""GPU: the soft-target cross entropy (mv_cross_entropy_soft) against torch's fp64 cross entropy on the explicit probability
target, mv_mix_batch against the index composition (CutMix, exact) and an fp64 evaluation (Mixup, to a derived bound), the
autograd wrappers, a micro ViT, and the engine's loop with and without the recipe keys.

Bars of the loss: those tests/test_hip_ops.py::test_cross_entropy_cls holds mv_cross_entropy to -- |loss - ref| < 1e-5 *
max(1, |ref|), relative L2 of dlogits < 1e-5, arg-max equal to torch's."""
import copy
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT, load_golden  # noqa: E402
from mixup_ref import (MIX_LAMS, MIX_SHAPES, ce_inputs, cutmix_boxes, cutmix_ref, mix_inputs, mixup_bound,  # noqa: E402
                       soft_target)

CE_SHAPES = [(1, 2), (2, 17), (3, 45), (8, 64), (5, 65), (4, 1000), (1031, 45)]
CE_PARAMS = [(1.0, 0.0), (1.0, 0.1), (0.3, 0.0), (0.3, 0.1), (0.0, 0.1)]
TOL = 1e-5


@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops as o
    return o


def rel_l2(got, want):
    return float((got.double().cpu() - want).norm() / want.norm().clamp_min(1e-300))


def close(got, want):
    return abs(got - want) < TOL * max(1.0, abs(want))


def fp64_reference(logits, labels, lam, eps):
    """-> (mean loss, per-sample losses, d mean / d logits), all fp64, from torch's cross entropy with probability targets."""
    z = logits.double().requires_grad_()
    t = soft_target(labels, logits.shape[1], lam, eps)
    per = torch.nn.functional.cross_entropy(z, t, reduction="none")
    mean = torch.nn.functional.cross_entropy(z, t)
    mean.backward()
    return float(mean.detach()), per.detach(), z.grad


# ================================================================== the loss kernel
@pytest.mark.parametrize("lam,eps", CE_PARAMS)
@pytest.mark.parametrize("B,C", CE_SHAPES)
def test_soft_cross_entropy_against_fp64(ops, B, C, lam, eps):
    logits, labels = ce_inputs(B, C)
    want, want_per, want_grad = fp64_reference(logits, labels, lam, eps)
    loss, dl, am, per = ops.cross_entropy_soft(logits.cuda(), labels.cuda(), lam, eps, want_grad=True, want_argmax=True)
    got, got_per, e_grad = float(loss), per.double().cpu(), rel_l2(dl, want_grad)
    e_per = float(((got_per - want_per).abs() / want_per.abs().clamp_min(1.0)).max())
    rowsum = float(dl.double().sum(1).abs().max().cpu())
    print(f"B={B} C={C} lam={lam} eps={eps}: loss {got:.8f} ref {want:.8f}; per-sample {e_per:.2e}; dlogits {e_grad:.2e}; "
          f"row sum {rowsum:.2e} of {C * 2.0 ** -23 / B:.2e}")
    assert close(got, want)
    assert e_per < TOL
    assert e_grad < TOL
    assert torch.equal(am.cpu(), logits.argmax(1))
    # softmax and target both sum to 1: what is left is the fp32 rounding of C terms
    assert rowsum <= C * 2.0 ** -23 * 1.0 / B


def test_soft_cross_entropy_wide_rows(ops):
    """C = 32 768 (the widest row the entry point promises) and a C that is no multiple of the wave."""
    for B, C in ((2, 32768), (3, 4099)):
        logits, labels = ce_inputs(B, C)
        want, want_per, want_grad = fp64_reference(logits, labels, 0.3, 0.1)
        loss, dl, am, per = ops.cross_entropy_soft(logits.cuda(), labels.cuda(), 0.3, 0.1, want_grad=True, want_argmax=True)
        assert close(float(loss), want) and rel_l2(dl, want_grad) < TOL and torch.equal(am.cpu(), logits.argmax(1))
        assert float(((per.double().cpu() - want_per).abs() / want_per.abs().clamp_min(1.0)).max()) < TOL


@pytest.mark.parametrize("B,C", [(8, 64), (5, 65), (1031, 45)])
def test_plain_case_agrees_with_cross_entropy(ops, B, C):
    logits, labels = ce_inputs(B, C)
    lg, lb = logits.cuda(), labels.cuda()
    loss0, dl0, am0 = ops.cross_entropy(lg, lb, want_grad=True, want_argmax=True)
    for pair_flip in (True, False):
        loss, dl, am, _ = ops.cross_entropy_soft(lg, lb, 1.0, 0.0, pair_flip=pair_flip, want_grad=True, want_argmax=True)
        assert close(float(loss), float(loss0))
        assert rel_l2(dl, dl0.double().cpu()) < TOL
        assert torch.equal(am, am0)


def test_label_smoothing_alone_is_torchs_label_smoothing(ops):
    logits, labels = ce_inputs(8, 64)
    want = float(torch.nn.functional.cross_entropy(logits.double(), labels, label_smoothing=0.1))
    for pair_flip in (True, False):
        assert close(float(ops.cross_entropy_soft(logits.cuda(), labels.cuda(), 1.0, 0.1, pair_flip=pair_flip)[0]), want)


def test_large_logits_stay_finite(ops):
    logits, labels = ce_inputs(5, 65)
    logits = torch.where(logits > 0, torch.full_like(logits, 80.0), torch.full_like(logits, -80.0))
    want, _, want_grad = fp64_reference(logits, labels, 0.3, 0.1)
    loss, dl, _, per = ops.cross_entropy_soft(logits.cuda(), labels.cuda(), 0.3, 0.1, want_grad=True)
    assert torch.isfinite(loss).all() and torch.isfinite(dl).all() and torch.isfinite(per).all()
    assert close(float(loss), want) and rel_l2(dl, want_grad) < TOL


@pytest.mark.parametrize("bad", [45, -1])
def test_a_label_outside_the_classes_poisons_the_loss(ops, bad):
    logits, labels = ce_inputs(5, 45)
    labels[1] = bad                                                              # sample 1, partner of sample 3
    loss, dl, am, per = ops.cross_entropy_soft(logits.cuda(), labels.cuda(), 0.3, 0.1, want_grad=True, want_argmax=True)
    torch.cuda.synchronize()                                                     # no fault
    assert torch.isnan(loss).all()
    assert torch.isnan(per).cpu().tolist() == [False, True, False, True, False]  # the sample and its partner, no other
    assert torch.isfinite(dl).all() and not dl[1].any() and not dl[3].any() and dl[0].any()
    assert torch.equal(am.cpu(), logits.argmax(1))
    # without a partner only the sample itself
    _, _, _, per = ops.cross_entropy_soft(logits.cuda(), labels.cuda(), 1.0, 0.1, pair_flip=False)
    assert torch.isnan(per).cpu().tolist() == [False, True, False, False, False]


def test_two_runs_are_bit_identical_and_grad_scale_is_exact(ops):
    logits, labels = ce_inputs(1031, 45)
    lg, lb = logits.cuda(), labels.cuda()
    a = ops.cross_entropy_soft(lg, lb, 0.3, 0.1, want_grad=True, want_argmax=True)
    b = ops.cross_entropy_soft(lg, lb, 0.3, 0.1, want_grad=True, want_argmax=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    h = ops.cross_entropy_soft(lg, lb, 0.3, 0.1, want_grad=True, grad_scale=0.5)
    assert torch.equal(h[0], a[0]) and torch.equal(h[3], a[3])
    assert torch.equal(h[1], a[1] * 0.5)                                          # a power of two: halves every element exactly
    assert float(h[1].double().sum(1).abs().max()) <= 45 * 2.0 ** -23 * 0.5 / 1031


def test_rejections_name_the_wrapper(ops):
    logits, labels = ce_inputs(4, 8)
    lg, lb = logits.cuda(), labels.cuda()
    cases = [dict(logits=lg[:, :1], labels=lb),                                  # C < 2
             dict(logits=lg, labels=lb, smoothing=-0.1), dict(logits=lg, labels=lb, smoothing=1.0),
             dict(logits=lg, labels=lb, lam=-0.1), dict(logits=lg, labels=lb, lam=1.5),
             dict(logits=lg, labels=lb, lam=0.5, pair_flip=False)]
    for kw in cases:
        with pytest.raises(RuntimeError, match="cross_entropy_soft"):
            ops.cross_entropy_soft(**kw)
    # what no tensor can express goes to the entry point directly: B < 0 and the null pointers
    from myrtle_vision.hip.lib import check, lib
    p = lambda t: t.data_ptr()
    loss, ws = torch.empty(1, device="cuda"), torch.empty(4, device="cuda")
    for args in ((p(lg), p(lb), p(loss), p(ws), None, None, -1, 8), (None, p(lb), p(loss), p(ws), None, None, 4, 8),
                 (p(lg), None, p(loss), p(ws), None, None, 4, 8), (p(lg), p(lb), None, p(ws), None, None, 4, 8),
                 (p(lg), p(lb), p(loss), None, None, None, 4, 8)):
        with pytest.raises(RuntimeError, match="cross_entropy_soft"):
            check(lib().mv_cross_entropy_soft(*args, 1.0, 0.0, 1, 1.0, None), "cross_entropy_soft")
    empty = ops.cross_entropy_soft(lg[:0], lb[:0], 0.3, 0.1, want_grad=True)      # B == 0: a no-op that succeeds
    assert empty[1].shape == (0, 8)
    x = torch.zeros(2, 3, 8, 8, device="cuda")
    for kw in (dict(box=(0, 9, 0, 2)), dict(box=(3, 2, 0, 2)), dict(box=(0, 2, 0, 9)), dict(box=(0, 2, -1, 2)), dict(lam=1.5)):
        with pytest.raises(RuntimeError, match="mix_batch"):
            ops.mix_batch(x, **kw)
    with pytest.raises(RuntimeError, match="mix_batch"):
        ops.mix_batch(torch.zeros(2 * 3 * 8 * 8 + 1, device="cuda")[1:].view(2, 3, 8, 8), lam=0.5)      # 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match="mix_batch"):
        ops.mix_batch(x.half(), lam=0.5)
    with pytest.raises(ValueError):
        ops.mix_batch(x)
    assert not x.any()


# ================================================================== mix_batch
GUARD = 64                                                                       # elements on each side: keeps the batch 16-byte aligned
SENTINEL = -512.0                                                                # exact in bf16


class Guarded:
    """A batch inside a larger allocation whose guard zones hold a sentinel."""

    def __init__(self, x):
        self.buf = torch.full((x.numel() + 2 * GUARD,), SENTINEL, dtype=x.dtype, device="cuda")
        self.x = self.buf[GUARD:GUARD + x.numel()].view(x.shape)
        self.x.copy_(x)
        assert self.x.data_ptr() % 16 == 0 and self.x.is_contiguous()

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cutmix_is_the_index_composition(ops, shape, dtype):
    x = mix_inputs(shape, dtype)
    B, _, H, W = shape
    for name, box in cutmix_boxes(H, W).items():
        g = Guarded(x)
        assert ops.mix_batch(g.x, box=box) is g.x
        want = cutmix_ref(x, box)
        assert torch.equal(bits(g.x), bits(want)), name
        assert g.guards_intact(), name
        if B % 2:
            assert torch.equal(bits(g.x[B // 2]), bits(x[B // 2])), name          # the middle sample is its own partner
        if name.startswith("empty"):
            assert torch.equal(bits(g.x), bits(x))
        if name == "whole":
            assert torch.equal(bits(g.x), bits(x.flip(0)))                       # the samples swap


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mixup_stays_inside_the_rounding_bound(ops, shape, dtype):
    x = mix_inputs(shape, dtype)
    B = shape[0]
    g = Guarded(x)
    ops.mix_batch(g.x, lam=1.0)
    assert torch.equal(bits(g.x), bits(x)) and g.guards_intact()                 # lam = 1: every bit stays
    ops.mix_batch(g.x, lam=0.0)
    assert torch.equal(g.x.cpu(), x.flip(0)) and g.guards_intact()               # lam = 0: the samples swap exactly
    for lam in MIX_LAMS:
        g = Guarded(x)
        ops.mix_batch(g.x, lam=lam)
        exact, bound = mixup_bound(x, lam)
        err = (g.x.double().cpu() - exact).abs()
        print(f"{shape} {dtype} lam={lam}: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all())
        assert g.guards_intact()
        if B % 2:
            assert torch.equal(bits(g.x[B // 2]), bits(x[B // 2]))


def test_mixup_on_every_alignment_of_a_pair(ops):
    """(2, 1, 7, 9): 63 elements per sample put the two samples of the pair at different offsets from a 16-byte boundary, so it goes
    element by element.  B = 7 with 1 100 001 fp32 (100 002 bf16) elements per sample: the pair (1, 5) sits at the same non-zero
    offset -- elements in front of the first boundary, a 16-byte body (fp32: longer than one pass of the grid), elements behind
    the last whole group -- while the pairs (0, 6) and (2, 4) sit at different offsets."""
    for shape, dtype in (((2, 1, 7, 9), torch.float32), ((2, 1, 7, 9), torch.bfloat16), ((7, 1, 1, 1100001), torch.float32),
                         ((7, 1, 1, 100002), torch.bfloat16)):
        x = mix_inputs(shape, dtype)
        g = Guarded(x)
        ops.mix_batch(g.x, lam=0.3)
        exact, bound = mixup_bound(x, 0.3)
        assert bool(((g.x.double().cpu() - exact).abs() <= bound).all()) and g.guards_intact()
        if shape[0] % 2:
            assert torch.equal(bits(g.x[shape[0] // 2]), bits(x[shape[0] // 2]))


# ================================================================== autograd
def test_autograd_matches_fp64(ops):
    from myrtle_vision.hip import functional as F
    logits, labels = ce_inputs(5, 65)
    want, _, want_grad = fp64_reference(logits, labels, 0.3, 0.1)
    for factor in (1.0, 2.0):
        lg = logits.cuda().requires_grad_()
        loss = F.soft_cross_entropy(lg, labels.cuda(), lam=0.3, smoothing=0.1)
        assert loss.dim() == 0 and close(float(loss.detach()), want)
        (loss * factor).backward()
        assert rel_l2(lg.grad, want_grad * factor) < TOL
    lg = logits.cuda().requires_grad_()
    crit = F.SoftTargetCrossEntropy(smoothing=0.1, return_argmax=True)
    loss, am = crit(lg, labels.cuda(), 0.3)
    assert not am.requires_grad and torch.equal(am.cpu(), logits.argmax(1))
    loss.backward()
    assert rel_l2(lg.grad, want_grad) < TOL
    assert type(F.CrossEntropyLoss()) is not type(crit) and not isinstance(crit, F.CrossEntropyLoss)


# ================================================================== a micro ViT
def test_micro_vit_gradients_match_torchs_loss_on_the_same_logits(ops):
    """micro_cls of tests/test_vit_parity.py (classification, fp32) at B = 4, one batch mixed with a fixed lam and box.  The
    parameter gradients from SoftTargetCrossEntropy against those from the loss torch evaluates (fp64, explicit [B, C] target) on
    the same HIP logits; both backward passes run through the same HIP model."""
    from myrtle_vision.hip.functional import SoftTargetCrossEntropy
    from myrtle_vision.models.vit import ViT
    from oracle.detinit import det_images, det_labels, det_param
    _, meta = load_golden("micro_cls")
    kw = dict(meta["kwargs"])
    vit = ViT(patch_size=16, q_format="FP32", precision="fp32", **kw)
    vit.load_state_dict({k: det_param(k, v.shape) for k, v in vit.state_dict().items()})
    vit = vit.cuda().train()
    img = det_images("mixup_model", 4, kw["image_size"]).cuda()
    labels = det_labels("mixup_model", (4,), kw["num_classes"]).cuda()
    H = W = kw["image_size"]
    box = (40, 150, 61, 200)
    lam, eps = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / (H * W), 0.1
    plain = img.clone()
    ops.mix_batch(img, box=box)
    assert torch.equal(img.cpu(), cutmix_ref(plain.cpu(), box))

    def grads(loss_of_logits):
        for p in vit.parameters():
            p.grad = None
        loss = loss_of_logits(vit(img))
        loss.backward()
        return float(loss), {n: p.grad.detach().double().cpu() for n, p in vit.named_parameters() if p.grad is not None}

    l_hip, g_hip = grads(lambda z: SoftTargetCrossEntropy(eps)(z, labels, lam))
    t = soft_target(labels.cpu(), kw["num_classes"], lam, eps).cuda()
    l_ref, g_ref = grads(lambda z: torch.nn.functional.cross_entropy(z.double(), t))
    assert close(l_hip, l_ref)
    assert set(g_hip) == set(g_ref) and len(g_hip) > 20
    for name in g_ref:
        e = float((g_hip[name] - g_ref[name]).norm() / g_ref[name].norm().clamp_min(1e-300))
        assert e < TOL, (name, e)


# ================================================================== the engine's loop
def _engine_config(tmp_path, recipe):
    """ViT-Tiny at depth 2 on a synthetic RESISC-45 directory with 16 training images: two iterations at batch 8."""
    from myrtle_vision.datasets.synthetic import make_resisc45
    cfg = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_tiny.json")))
    data = json.load(open(os.path.join(ROOT, "classification", "data_configs", "data_config.json")))
    data["dataset_path"] = make_resisc45(str(tmp_path / "NWPU-RESISC45"), classes=12, per_class=2)
    dpath = str(tmp_path / "data_config.json")
    json.dump(data, open(dpath, "w"))
    cfg["data_config_path"] = dpath
    cfg["train_config"].update(output_directory=str(tmp_path / "ckpt"), epochs=1, local_batch_size=8, global_batch_size=8,
                               iters_per_checkpoint=1000, iters_per_val=1000, distributed=False, pretrained_backbone=None)
    cfg["vit_config"]["depth"] = 2
    if recipe:
        mix = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_base_mixup.json")))["train_config"]
        cfg["train_config"].update({k: mix[k] for k in ("label_smoothing", "mixup_alpha", "cutmix_alpha")})
    return cfg


def _losses(out):
    return [float(l.split("loss=")[1].split()[0]) for l in out.splitlines() if l.startswith("Iteration")]


def test_engine_mixes_each_batch_and_keeps_the_labels(tmp_path, capsys, monkeypatch):
    from myrtle_vision.engine import train_worker
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.mixup import Mixup
    seen, fed = [], []
    mix_call, vit_forward = Mixup.__call__, ViT.forward

    def recording_mix(self, imgs, labels):
        before, labels_before = imgs.clone(), labels.clone()
        out, lam = mix_call(self, imgs, labels)
        seen.append((before, out.clone(), lam, torch.equal(labels, labels_before)))
        return out, lam

    def recording_forward(self, x, *a, **kw):
        if self.training:
            fed.append(x.clone())
        return vit_forward(self, x, *a, **kw)

    monkeypatch.setattr(Mixup, "__call__", recording_mix)
    monkeypatch.setattr(ViT, "forward", recording_forward)
    iters = train_worker(0, 1, copy.deepcopy(_engine_config(tmp_path, recipe=True)), "classification")
    out = capsys.readouterr().out
    losses = _losses(out)
    assert iters == 2 and len(losses) == 2 and all(l == l and abs(l) < 50 for l in losses) and "nan" not in out.lower()
    accs = [float(l.split("acc=")[1]) for l in out.splitlines() if l.startswith("Iteration")]
    assert all(a * 8 == round(a * 8) and 0 <= a <= 1 for a in accs)               # hits among the 8 ORIGINAL labels
    assert len(seen) == 2 and len(fed) == 2
    for (before, after, lam, labels_same), x in zip(seen, fed):
        assert labels_same                                                       # the labels tensor is not touched
        assert torch.equal(x, after)                                             # the model is handed the mixed batch
        assert torch.equal(before, after) == (lam == 1.0)                        # lam == 1 exactly when nothing was mixed
        assert 0.0 <= lam <= 1.0
    assert any(not torch.equal(b, a) for b, a, _, _ in seen)


def test_engine_without_the_keys_never_imports_the_mixer(tmp_path, capsys, monkeypatch):
    from myrtle_vision.engine import train_worker
    from myrtle_vision.hip import functional as F

    def never(*a, **kw):
        raise AssertionError("the soft-target path ran without a recipe key")

    monkeypatch.setattr(F.SoftTargetCrossEntropy, "forward", never)
    monkeypatch.setattr(F, "soft_cross_entropy", never)
    monkeypatch.delitem(sys.modules, "myrtle_vision.utils.mixup", raising=False)
    iters = train_worker(0, 1, copy.deepcopy(_engine_config(tmp_path, recipe=False)), "classification")
    assert "myrtle_vision.utils.mixup" not in sys.modules
    losses = _losses(capsys.readouterr().out)
    assert iters == 2 and len(losses) == 2 and all(l == l for l in losses)
