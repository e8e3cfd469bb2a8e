"""GPU: ``mv_adamw_table`` -- one AdamW launch over the whole arena with a learning-rate scale and a weight decay per tensor and a
weight EMA -- against the existing kernel (bit for bit), against ``torch.optim.AdamW`` with one group per tensor (the project's
AdamW bar), inside a captured step, through ``ema_weights()`` and through the training loop."""
import copy
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT, load_golden  # noqa: E402
from optim_table_ref import BAR, Reference, edge_arena, flat, gap_mask, relerr  # noqa: E402

PAD = 64                                                     # canary elements on either side of every array (256 bytes)
CANARY = -12345.5


@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops as _ops
    _ops.lib()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return _ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def _framed(host):
    """A device copy of ``host`` with PAD canary elements before and after it -> (whole buffer, the array's view)."""
    buf = torch.full((host.numel() + 2 * PAD,), CANARY, dtype=host.dtype)
    buf[PAD:PAD + host.numel()] = host
    buf = buf.cuda()
    return buf, buf[PAD:PAD + host.numel()]


def _canaries_intact(buf):
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())


def _items(sizes, offsets, pairs):
    from myrtle_vision.utils.optim import build_items
    off, length, seg, segments = build_items(offsets, sizes, pairs)
    items = (torch.tensor(off, dtype=torch.int64).cuda(), torch.tensor(length, dtype=torch.int32).cuda(),
             torch.tensor(seg, dtype=torch.int32).cuda())
    return items, torch.tensor([s for s, _ in segments]).cuda(), torch.tensor([w for _, w in segments]).cuda()


# ---------------------------------------------------------------- bit equality with the existing kernel
@pytest.mark.parametrize("scalars", ["launch", "device"])
def test_table_launch_equals_two_adamw_launches_bit_for_bit(ops, scalars):
    """All scales 1, the two existing weight decays, no EMA: p, m, v of ONE mv_adamw_table launch equal those of the two mv_adamw
    launches (decay region, no-decay region) over the same arena, over three steps.  The sizes put tensor tails (the scalar path of
    the table kernel) where the existing kernel runs its float4 path."""
    sizes, offs, total = edge_arena(40)
    n_decay_tensors = 22
    nd = offs[n_decay_tensors]
    tensors = [torch.randn(n, generator=g(10 + i)) for i, n in enumerate(sizes)]
    p0 = flat(tensors, offs, total)
    pairs = [(1.0, 0.05 if i < n_decay_tensors else 0.0) for i in range(len(sizes))]
    items, seg_scale, seg_wd = _items(sizes, offs, pairs)
    gaps = gap_mask(offs, sizes, total).cuda()
    pa, ma, va = p0.clone().cuda(), torch.zeros(total).cuda(), torch.zeros(total).cuda()
    pb, mb, vb = p0.clone().cuda(), torch.zeros(total).cuda(), torch.zeros(total).cuda()
    coef = torch.tensor([0.8125]).cuda()
    kw = dict(beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=0.5, clip_coef=coef)
    for step in range(1, 4):
        lr = [1e-3, 7e-4, 3e-4][step - 1]
        grads = flat([torch.randn(n, generator=g(100 * step + i)) * (1 + i % 3) for i, n in enumerate(sizes)], offs, total).cuda()
        hyper = None
        if scalars == "device":
            hyper = torch.tensor([lr, 1.0 - 0.9 ** step, 1.0 - 0.999 ** step], dtype=torch.float32).cuda()
        for lo, hi, wd in ((0, nd, 0.05), (nd, total, 0.0)):
            ops.adamw_step(pa[lo:hi], grads[lo:hi], ma[lo:hi], va[lo:hi], lr=lr, weight_decay=wd, step=step, hyper=hyper, **kw)
        ops.adamw_table_step(pb, grads, mb, vb, items, seg_scale, seg_wd, lr=lr, step=step, hyper=hyper, **kw)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), step
    assert not bool(pb[gaps].any()) and not bool(mb[gaps].any()) and not bool(vb[gaps].any())
    assert not torch.equal(pb, p0.cuda())


# ---------------------------------------------------------------- edge shapes against torch, with guard zones
def _edge_case():
    sizes, offs, total = edge_arena(40)
    scales = [0.75 ** (i % 5) for i in range(len(sizes))]                       # 5 distinct scales
    wds = [0.05 if (i // 5) % 2 == 0 else 0.0 for i in range(len(sizes))]       # 2 weight decays
    tensors = [torch.randn(n, generator=g(500 + i)) for i, n in enumerate(sizes)]
    grads = [[torch.randn(n, generator=g(1000 * s + i)) * (0.1 + i % 4) for i, n in enumerate(sizes)] for s in range(3)]
    return sizes, offs, total, scales, wds, tensors, grads


EDGE_LRS = [1e-3, 6e-4, 2.5e-4]
EDGE_COEF, EDGE_GSCALE, EDGE_DECAY = 0.625, 0.5, 0.9


@pytest.fixture(scope="module")
def edge_reference():
    """torch.optim.AdamW, one group per tensor, and the fp64 EMA: computed once, shared, left unchanged."""
    sizes, offs, total, scales, wds, tensors, grads = _edge_case()
    ref = Reference(tensors, scales, wds, ema_decay=EDGE_DECAY)
    mult = torch.tensor(EDGE_GSCALE) * torch.tensor(EDGE_COEF)                  # fp32, as the kernel folds the two
    for s in range(3):
        ref.step(EDGE_LRS[s], [gr * mult for gr in grads[s]])
    return flat([p.detach() for p in ref.params], offs, total, torch.float64), flat(ref.ema, offs, total, torch.float64)


def _edge_run(ops):
    sizes, offs, total, scales, wds, tensors, grads = _edge_case()
    items, seg_scale, seg_wd = _items(sizes, offs, list(zip(scales, wds)))
    assert seg_scale.numel() == 10
    p0 = flat(tensors, offs, total)
    bufs = {k: _framed(h) for k, h in (("p", p0), ("m", torch.zeros(total)), ("v", torch.zeros(total)), ("ema", p0))}
    coef = torch.tensor([EDGE_COEF]).cuda()
    gbufs = []
    for s in range(3):
        gbuf, gr = _framed(flat(grads[s], offs, total))
        gbufs.append((gbuf, gbuf.clone()))
        ops.adamw_table_step(bufs["p"][1], gr, bufs["m"][1], bufs["v"][1], items, seg_scale, seg_wd, lr=EDGE_LRS[s], beta1=0.9,
                             beta2=0.999, eps=1e-8, step=s + 1, grad_scale=EDGE_GSCALE, clip_coef=coef, ema=bufs["ema"][1],
                             ema_decay=EDGE_DECAY)
    torch.cuda.synchronize()
    return bufs, gbufs, gap_mask(offs, sizes, total).cuda()


def test_edge_shapes_match_torch_and_leave_gaps_and_guard_zones_alone(ops, edge_reference):
    want_p, want_ema = edge_reference
    bufs, gbufs, gaps = _edge_run(ops)
    ep, ee = relerr(bufs["p"][1], want_p), relerr(bufs["ema"][1], want_ema)
    print(f"edge shapes: relative error p {ep:.3e}, ema {ee:.3e} (bar {BAR:g})")
    assert ep < BAR and ee < BAR
    sizes, offs, total = edge_arena(40)
    for k, (o, n) in enumerate(zip(offs, sizes)):                               # and per tensor: a small tensor is held to it too
        assert relerr(bufs["p"][1][o:o + n], want_p[o:o + n]) < BAR, (k, n)
        assert relerr(bufs["ema"][1][o:o + n], want_ema[o:o + n]) < BAR, (k, n)
    for name, (buf, arr) in bufs.items():
        assert _canaries_intact(buf), name
        assert bool((arr[gaps] == 0).all()), name                               # every gap element exactly 0
    for gbuf, before in gbufs:
        assert torch.equal(gbuf, before)                                        # the gradients are read only
    again, _, _ = _edge_run(ops)
    for name in bufs:
        assert torch.equal(bufs[name][0], again[name][0]), name                 # two runs, the same bits


# ---------------------------------------------------------------- model level
def _micro(seed=21):
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.utils import seed_everything
    _, meta = load_golden("micro_cls")
    seed_everything(seed)
    return ViT(patch_size=16, q_format="FP32", precision="bf16", **meta["kwargs"]).cuda().train(), meta["kwargs"]["num_classes"]


RECIPE = dict(layer_decay=0.75, no_weight_decay=["pos_embedding", "cls_token"], ema_decay=0.99)


def _table_opt(vit, **kw):
    from myrtle_vision.utils.optim import ParamArena, TableAdamW
    return TableAdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-3, weight_decay=0.05, **kw)


# Betas that fp32 holds exactly (1 - 2^-3, 1 - 2^-10).  The kernel forms 1 - beta2 in fp32 from the fp32 beta2, as adamw_kernel
# does and as bit equality with it demands; torch forms it in fp64 from the fp64 beta2 and rounds once.  For beta2 = 0.999 the two
# differ by 1.3e-5 relative (fp32(0.999) = 0.99900001287), every v carries that factor and every UPDATE its square root, 6.4e-6
# -- on both kernels, old and new.  Over an array of weights of order 1 that is far below the bar (what test_adamw_matches_torch
# measures); on a tensor that starts at zero (a LayerNorm or Linear bias) the weight IS the sum of the updates and the bar cannot
# hold: measured 6.7e-6 on transformer.layers.0.0.fn.norm.bias.  With exact betas both sides are handed the same numbers, and
# the per-tensor bar checks what this test is about -- each tensor's scale, weight decay, schedule and EMA -- at rounding level.
EXACT_BETAS = (0.875, 1.0 - 2.0 ** -10)
DEFAULT_BETAS = (0.9, 0.999)


@pytest.mark.parametrize("betas", [EXACT_BETAS, DEFAULT_BETAS], ids=["exact_betas", "default_betas"])
def test_micro_vit_follows_the_per_tensor_reference(betas):
    """Four optimizer steps of the micro ViT with layer decay 0.75, two exempt names, the EMA and a cosine schedule with warm-up,
    against torch.optim.AdamW with one group per tensor driven by the gradients the HIP model produced.  exact_betas: the bar PER
    TENSOR.  default_betas (0.9, 0.999): the bar over the whole arena, the measure it was taken from; per tensor the zero-initialised
    biases sit at 6.7e-6 there for the reason above (the figure is printed)."""
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.utils.optim import CosineLRScheduler, layer_scales
    vit, nc = _micro()
    opt = _table_opt(vit, betas=betas, **RECIPE)
    a = opt.arena
    assert len(opt.segments) > 4                                                # 4 scales x 2 decays, not all pairs occur
    scales, wds = layer_scales(a.names, 0.75), opt.tensor_weight_decays()
    assert scales == opt.lr_scales
    by = dict(zip(a.names, zip(scales, wds)))
    assert by["pos_embedding"] == (0.75 ** 3, 0.0) and by["patch_to_embedding.weight"] == (0.75 ** 3, 0.05)
    assert by["decoder.linear.weight"] == (1.0, 0.05) and by["decoder.linear.bias"] == (1.0, 0.0)
    ref = Reference([p.detach() for p in a.params], scales, wds, betas=betas, ema_decay=RECIPE["ema_decay"])
    sched = CosineLRScheduler(opt, t_initial=6, lr_min=1e-5, warmup_t=2, warmup_lr_init=1e-4)
    gen = g(3)
    used = []
    for k in range(4):
        x, y = torch.randn(4, 3, 224, 224, generator=gen).cuda(), torch.randint(0, nc, (4,), generator=gen).cuda()
        opt.zero_grad()
        cross_entropy(vit(x), y).backward()
        a.sync_grads()
        lr = opt.param_groups[0]["lr"]
        used.append(lr)
        ref.step(lr, [a.slot(j).clone() for j in range(len(a.params))])
        opt.step()
        sched.step(k + 1)
    assert used[0] == 1e-4 and used[0] < used[1] < 1e-3 and used[2] > used[3] > 1e-5        # warm-up, then the cosine
    torch.cuda.synchronize()
    sizes = [p.numel() for p in a.params]
    whole_p = relerr(a.flat_param, flat([p.detach() for p in ref.params], a.offsets, a.total, torch.float64))
    whole_e = relerr(opt.ema, flat(ref.ema, a.offsets, a.total, torch.float64))
    worst = (0.0, None)
    for j, (n, o, k) in enumerate(zip(a.names, a.offsets, sizes)):
        ep = relerr(a.flat_param[o:o + k], ref.params[j].detach().reshape(-1))
        ee = relerr(opt.ema[o:o + k], ref.ema[j].reshape(-1))
        worst = max(worst, (ep, n), (ee, n + " (ema)"))
    print(f"micro ViT, betas {betas}: whole arena p {whole_p:.3e} ema {whole_e:.3e}; worst tensor {worst[0]:.3e} at {worst[1]} "
          f"(bar {BAR:g})")
    assert whole_p < BAR and whole_e < BAR
    if betas == EXACT_BETAS:
        assert worst[0] < BAR, worst
    gaps = gap_mask(a.offsets, sizes, a.total).cuda()
    assert not bool(a.flat_param[gaps].any()) and not bool(opt.ema[gaps].any())


# ---------------------------------------------------------------- graph capture
def test_graphed_step_equals_eager_step_with_all_three_options():
    """tests/test_train_gpu.py's capture test on the table optimizer: replays with a learning-rate change in between give, bit for
    bit, the parameters, moments and EMA of the eager steps."""
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.graph import GraphedTrainStep
    from myrtle_vision.utils.utils import seed_everything
    kw = dict(image_size=224, patch_size=16, dim=128, depth=2, heads=2, mlp_dim=256, dropout=0.0, emb_dropout=0.0,
              decoder="classification", num_classes=10)
    loss_fn = lambda m, x, y: cross_entropy(m(x), y)
    gen = g(9)
    batches = [(torch.randn(4, 3, 224, 224, generator=gen).cuda(), torch.randint(0, 10, (4,), generator=gen).cuda()) for _ in range(4)]
    lrs = [1e-3, 1e-3, 4e-4, 7e-4]

    def build():
        seed_everything(21)
        vit = ViT(precision="bf16", q_format="FP32", **kw).cuda().train()
        opt = _table_opt(vit, **RECIPE)
        opt.max_grad_norm = 1.0                                              # the clip coefficient is a device scalar as well
        return vit, opt

    def set_lr(opt, lr):
        for grp in opt.param_groups:
            grp["lr"] = lr

    vit_e, opt_e = build()
    losses_e = []
    for i in [0, 0, 0, 1, 2, 3]:
        set_lr(opt_e, lrs[i])
        opt_e.zero_grad()
        loss = loss_fn(vit_e, *batches[i])
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss))
    vit_g, opt_g = build()
    graphed = GraphedTrainStep(vit_g, opt_g, loss_fn, *batches[0], warmup=3)
    assert opt_g.step_count == 3
    losses_g = []
    for i in (1, 2, 3):
        set_lr(opt_g, lrs[i])
        losses_g.append(float(graphed(*batches[i])))
    torch.cuda.synchronize()
    assert opt_g.step_count == opt_e.step_count == 6
    assert losses_g == losses_e[3:]
    assert torch.equal(opt_g.arena.flat_param, opt_e.arena.flat_param)
    assert torch.equal(opt_g.exp_avg, opt_e.exp_avg) and torch.equal(opt_g.exp_avg_sq, opt_e.exp_avg_sq)
    assert torch.equal(opt_g.ema, opt_e.ema) and not torch.equal(opt_g.ema, opt_g.arena.flat_param)
    vit_g.eval(), vit_e.eval()
    with torch.no_grad(), opt_g.ema_weights(), opt_e.ema_weights():
        assert torch.equal(vit_g(batches[0][0]), vit_e(batches[0][0]))


# ---------------------------------------------------------------- ema_weights()
def test_ema_weights_swaps_restores_and_matches_the_checkpoint_entry(tmp_path):
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.utils.models import load_checkpoint, save_checkpoint
    from myrtle_vision.utils.optim import CosineLRScheduler
    vit, nc = _micro()
    opt = _table_opt(vit, **dict(RECIPE, ema_decay=0.5))
    sched = CosineLRScheduler(opt, t_initial=6, lr_min=1e-5)
    gen = g(5)
    x, y = torch.randn(4, 3, 224, 224, generator=gen).cuda(), torch.randint(0, nc, (4,), generator=gen).cuda()
    for _ in range(2):
        opt.zero_grad()
        cross_entropy(vit(x), y).backward()
        opt.step()
    vit.eval()
    p0, e0 = opt.arena.flat_param.clone(), opt.ema.clone()
    assert not torch.equal(p0, e0)
    path = str(tmp_path / "ckpt")
    save_checkpoint(vit, opt, sched, 2, path, model_ema=opt.ema_state_dict(vit))
    with torch.no_grad():
        plain = vit(x).clone()
        with opt.ema_weights():
            assert torch.equal(opt.arena.flat_param, e0) and torch.equal(opt.ema, p0)        # exchanged, bit for bit
            inside = vit(x).clone()
            with pytest.raises(RuntimeError, match="ema_weights"):
                opt.step()
        assert torch.equal(opt.arena.flat_param, p0) and torch.equal(opt.ema, e0)            # and back
        assert torch.equal(vit(x), plain) and not torch.equal(inside, plain)                 # the weight copies followed both ways
        other, _ = _micro(seed=77)
        load_checkpoint(other, None, None, path, use_ema=True)
        other.eval()
        assert torch.equal(other(x), inside)


# ---------------------------------------------------------------- the training loop
def test_train_worker_with_the_three_keys(tmp_path, capsys):
    """Two iterations of the segmentation loop on the synthetic set: the checkpoints carry "model_ema", the EMA validation is logged
    beside the plain one under the same tags with an _ema suffix, and evaluation honours "use_ema"."""
    from myrtle_vision.datasets.synthetic import make_dlrsd
    from myrtle_vision.engine import evaluate, train_worker
    cfg = json.load(open(os.path.join(ROOT, "segmentation", "train_configs", "seg_tiny.json")))
    data = json.load(open(os.path.join(ROOT, "segmentation", "data_configs", "data_config.json")))
    data["dataset_path"] = make_dlrsd(str(tmp_path / "DLRSD_dataset"), count=32)
    cfg["data_config_path"] = str(tmp_path / "data_config.json")
    json.dump(data, open(cfg["data_config_path"], "w"))
    out_dir = str(tmp_path / "ckpt")
    cfg["train_config"].update(output_directory=out_dir, epochs=1, local_batch_size=8, global_batch_size=8, iters_per_checkpoint=1,
                               iters_per_val=1, distributed=False, pretrained_backbone=None, tensorboard_dir=str(tmp_path / "runs"),
                               layer_decay=0.75, no_weight_decay=["pos_embedding", "cls_token"], model_ema_decay=0.5)
    cfg["vit_config"]["depth"] = 2
    iters = train_worker(0, 1, copy.deepcopy(cfg), "segmentation")
    out = capsys.readouterr().out
    assert iters == 2 and "nan" not in out.lower()
    assert "val_loss_ema" in out and "val_acc_ema" in out and "val_miou_ema" in out
    logged = os.listdir(cfg["train_config"]["tensorboard_dir"])
    assert logged, "validation scalars were not written"
    if "scalars.jsonl" in logged:
        rows = [json.loads(l) for l in open(os.path.join(cfg["train_config"]["tensorboard_dir"], "scalars.jsonl"))]
        assert {r["tag"] for r in rows} == {"accuracy", "loss", "miou", "accuracy_ema", "loss_ema", "miou_ema"}
        assert {r["step"] for r in rows if r["tag"].endswith("_ema")} == {0, 1}
    ck = torch.load(os.path.join(out_dir, "vit_000001"), map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "iteration", "model_ema"}
    assert ck["optimizer"]["layer_decay"] == 0.75 and ck["optimizer"]["no_weight_decay"] == ["pos_embedding", "cls_token"]
    assert list(ck["model_ema"]) == list(ck["model"])
    w = "transformer.layers.0.0.fn.fn.to_qkv.weight"
    assert not torch.equal(ck["model_ema"][w], ck["model"][w])                   # one step at decay 0.5: half way
    ck0 = torch.load(os.path.join(out_dir, "vit_000000"), map_location="cpu", weights_only=False)
    assert all(torch.equal(ck0["model_ema"][k], ck0["model"][k]) for k in ck0["model"])       # it starts from the weights
    cfg2 = copy.deepcopy(cfg)
    cfg2["train_config"]["checkpoint_path"] = os.path.join(out_dir, "vit_000001")
    cfg2["use_ema"] = True
    res = evaluate(cfg2, "segmentation")
    assert 0.0 <= res["accuracy"] <= 1.0


def test_detection_loop_with_the_three_keys(tmp_path, capsys):
    """The detection loop (tests/test_detection_data_gpu.py's configuration): the epoch's validation also runs on the EMA and is
    logged beside the plain figures, the checkpoint carries "model_ema" and evaluation honours "use_ema"."""
    import math
    from myrtle_vision.datasets.synthetic import make_dior_coco
    from myrtle_vision.engine import evaluate, train_worker
    cfg = json.load(open(os.path.join(ROOT, "detection", "train_configs", "yolos_tiny.json")))
    data = json.load(open(os.path.join(ROOT, "detection", "data_configs", "data_config.json")))
    data["dataset_path"] = make_dior_coco(str(tmp_path / "DIOR-COCO"), counts=(4, 2, 2))
    data.update(train_subset=None, valid_subset=None)
    ratio = {"max_size_ratio": [4, 3]}
    norm = {"Normalize": {"Mean": [0.5] * 3, "Std": [0.5] * 3}}
    data["transform_ops_train"] = {"RandomHorizontalFlip": None, "RandomResize": {"scales": [64, 80], **ratio}, **norm}
    data["transform_ops_val"] = {"RandomResize": {"scales": [96], **ratio}, **norm}
    cfg["data_config_path"] = str(tmp_path / "data_config.json")
    json.dump(data, open(cfg["data_config_path"], "w"))
    out_dir = str(tmp_path / "ckpt")
    cfg["train_config"].update(output_directory=out_dir, epochs=1, local_batch_size=2, global_batch_size=2, distributed=False,
                               pretrained_backbone=None, layer_decay=0.75, no_weight_decay=["pos_embedding", "cls_token"],
                               model_ema_decay=0.5)
    cfg["vit_config"].update(embed_dim=64, depth=2, heads=1, mlp_dim=128, num_det_tokens=10, precision="fp32")
    assert train_worker(0, 1, copy.deepcopy(cfg), "detection") == 2
    rows = [json.loads(line) for line in open(os.path.join(out_dir, "train_log.jsonl"))]
    epochs = [r for r in rows if "epoch" in r]
    assert len(epochs) == 1 and math.isfinite(epochs[0]["val_loss_ema"]) and 0.0 <= epochs[0]["ap_ema"] <= 1.0
    assert math.isfinite(epochs[0]["val_loss"]) and epochs[0]["val_loss_ema"] != epochs[0]["val_loss"]
    ck = torch.load(os.path.join(out_dir, "vit_epoch0"), map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "iteration", "model_ema"} and ck["iteration"] == 2
    cfg2 = copy.deepcopy(cfg)
    cfg2["train_config"].update(checkpoint_path=os.path.join(out_dir, "vit_epoch0"), use_ema=True)
    res = evaluate(cfg2, "detection")
    assert len(res["stats"]) == 12 and 0.0 <= res["AP"] <= 1.0
    assert "nan" not in capsys.readouterr().out.lower()
