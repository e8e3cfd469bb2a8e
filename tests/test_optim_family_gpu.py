"""GPU: ``mv_sgd_table`` and ``mv_lamb_table`` -- SGD against ``torch.optim.SGD`` with one group per tensor (the project's optimizer bar),
LAMB against the fp64 evaluation of its formulas (8 x the error of torch's own fp32 evaluation of them, measured in this run, never
below the bar), LAMB's branches, bit-level determinism of its per-tensor reduction, both inside a captured step, LAMB against the
existing AdamW kernel where every trust ratio is 1, and both through a training loop.

With MV_OPTIM_FAMILY_PARITY_OUT set, the LAMB test writes every tensor's baseline, bar and measured errors to that file
(profiles/optim_family_parity.txt is such a run)."""
import copy
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402
from optim_family_ref import BAR, BIG, LambReference, SGDReference, arena_offsets, edge_arena, f32, flat, gap_mask, lamb_bars, relerr  # noqa: E402

PAD = 64                                                     # canary elements on either side of every array (256 bytes)
CANARY = -12345.5
LRS = [1e-3, 6e-4, 2.5e-4]
COEF, GSCALE, DECAY = 0.625, 0.5, 0.9


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


def _tables(sizes, offsets, pairs):
    """The device tables of one arena: (items, seg_lr_scale, seg_wd, item_tensor, tensor_range)."""
    from myrtle_vision.utils.optim import build_item_tensors, build_items
    off, length, seg, segments = build_items(offsets, sizes, pairs)
    items = (torch.tensor(off, dtype=torch.int64).cuda(), torch.tensor(length, dtype=torch.int32).cuda(),
             torch.tensor(seg, dtype=torch.int32).cuda())
    item_tensor, first, count = build_item_tensors(sizes)
    return (items, torch.tensor([s for s, _ in segments]).cuda(), torch.tensor([w for _, w in segments]).cuda(),
            torch.tensor(item_tensor, dtype=torch.int32).cuda(), torch.tensor(list(zip(first, count)), dtype=torch.int32).cuda())


@functools.lru_cache(maxsize=None)
def _case(big):
    """The edge arena (40 tensors of 1 ... 70 001 elements; ``big``: one more of 256 * 4096 + 1), 5 scales x 2 weight decays, weights
    and three steps' gradients.  Built once, shared, left unchanged."""
    sizes, _, _ = edge_arena(40)
    sizes = list(sizes) + ([BIG] if big else [])
    offs, total = arena_offsets(sizes)
    scales = [0.75 ** (i % 5) for i in range(len(sizes))]
    wds = [0.05 if (i // 5) % 2 == 0 else 0.0 for i in range(len(sizes))]
    tensors = [torch.randn(n, generator=g(700 + i)) for i, n in enumerate(sizes)]
    grads = [[torch.randn(n, generator=g(2000 * (s + 1) + i)) * (0.1 + i % 4) for i, n in enumerate(sizes)] for s in range(3)]
    return sizes, offs, total, scales, wds, tensors, grads


def _mult():
    return torch.tensor(GSCALE) * torch.tensor(COEF)         # fp32, as the kernels fold grad_scale and the clip coefficient


def _ema64(ema, params):
    d = f32(DECAY)
    return [d * e + (1.0 - d) * p.detach().double() for e, p in zip(ema, params)]


# ---------------------------------------------------------------- SGD on the edge arena
@functools.lru_cache(maxsize=None)
def _sgd_reference(mu, nesterov):
    sizes, offs, total, scales, wds, tensors, grads = _case(False)
    ref = SGDReference(tensors, scales, wds, mu, nesterov)
    ema = [t.double() for t in tensors]
    for s in range(3):
        ref.step(LRS[s], [gr * _mult() for gr in grads[s]])
        ema = _ema64(ema, ref.params)
    bufs = ref.buffers()
    return ([p.detach().double() for p in ref.params], None if mu == 0 else [b.double() for b in bufs], ema)


@pytest.mark.parametrize("mu,nesterov", [(0.0, False), (0.9, False), (0.9, True)], ids=["plain", "momentum", "nesterov"])
def test_sgd_edge_shapes_match_torch_and_leave_gaps_and_guard_zones_alone(ops, mu, nesterov):
    sizes, offs, total, scales, wds, tensors, grads = _case(False)
    want_p, want_b, want_e = _sgd_reference(mu, nesterov)
    items, seg_scale, seg_wd, _, _ = _tables(sizes, offs, list(zip(scales, wds)))
    assert seg_scale.numel() == 10
    p0 = flat(tensors, offs, total)
    bufs = {"p": _framed(p0), "ema": _framed(p0)}
    if mu != 0:
        bufs["buf"] = _framed(torch.zeros(total))
    coef = torch.tensor([COEF]).cuda()
    gbufs = []
    for s in range(3):
        gbuf, gr = _framed(flat(grads[s], offs, total))
        gbufs.append((gbuf, gbuf.clone()))
        ops.sgd_table_step(bufs["p"][1], gr, bufs["buf"][1] if mu != 0 else None, items, seg_scale, seg_wd, lr=LRS[s], momentum=mu,
                           nesterov=nesterov, grad_scale=GSCALE, clip_coef=coef, ema=bufs["ema"][1], ema_decay=DECAY)
    torch.cuda.synchronize()
    worst = {}
    for name, want in (("p", want_p), ("buf", want_b), ("ema", want_e)):
        if want is None:
            assert name not in bufs                                             # mu == 0: no buffer exists, none was passed
            continue
        errs = [relerr(bufs[name][1][o:o + n], want[k].reshape(-1)) for k, (o, n) in enumerate(zip(offs, sizes))]
        worst[name] = max(errs)
        print(f"sgd mu={mu} nesterov={nesterov}: worst tensor {name} {worst[name]:.3e} (bar {BAR:g})")
    for name, w in worst.items():
        assert w < BAR, (name, w)
    gaps = gap_mask(offs, sizes, total).cuda()
    for name, (buf, arr) in bufs.items():
        assert _canaries_intact(buf), name
        assert bool((arr[gaps] == 0).all()), name                               # every gap element exactly 0
    for gbuf, before in gbufs:
        assert torch.equal(gbuf, before)                                        # the gradients are read only


def test_sgd_device_rate_equals_launch_rate_bit_for_bit(ops):
    """hyper[0] on the device (what a captured launch reads) against the same rate as a launch argument."""
    sizes, offs, total, scales, wds, tensors, grads = _case(False)
    items, seg_scale, seg_wd, _, _ = _tables(sizes, offs, list(zip(scales, wds)))
    gr = flat(grads[0], offs, total).cuda()
    out = []
    for hyper in (None, torch.tensor([LRS[1], 7.0, 7.0]).cuda()):               # entries 1 and 2 are not read
        p, b = flat(tensors, offs, total).cuda(), torch.zeros(total).cuda()
        ops.sgd_table_step(p, gr, b, items, seg_scale, seg_wd, lr=LRS[1], momentum=0.9, nesterov=True, hyper=hyper)
        out.append((p, b))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---------------------------------------------------------------- LAMB on the edge arena plus one tensor of 257 items
@functools.lru_cache(maxsize=None)
def _lamb_reference():
    sizes, offs, total, scales, wds, tensors, grads = _case(True)
    r64, r32 = LambReference(tensors, scales, wds), LambReference(tensors, scales, wds, dtype=torch.float32)
    ema = [t.double() for t in tensors]
    for s in range(3):
        r64.step(LRS[s], [gr * _mult() for gr in grads[s]])
        r32.step(LRS[s], [gr * _mult() for gr in grads[s]])
        ema = _ema64(ema, r64.p)
    return r64, lamb_bars(r64, r32), ema


def _lamb_run(ops, sizes, offs, total, pairs, tensors, grads, ema=True, **kw):
    items, seg_scale, seg_wd, item_tensor, tensor_range = _tables(sizes, offs, pairs)
    p0 = flat(tensors, offs, total)
    bufs = {k: _framed(h) for k, h in (("p", p0), ("m", torch.zeros(total)), ("v", torch.zeros(total)), ("ema", p0))}
    ws = ops.lamb_workspace(items[0].numel(), torch.device("cuda"))
    gbufs = []
    for s, step_grads in enumerate(grads):
        gbuf, gr = _framed(flat(step_grads, offs, total))
        gbufs.append((gbuf, gbuf.clone()))
        ops.lamb_table_step(bufs["p"][1], gr, bufs["m"][1], bufs["v"][1], items, item_tensor, tensor_range, seg_scale, seg_wd, ws,
                            lr=LRS[s], beta1=0.9, beta2=0.999, eps=1e-6, step=s + 1, ema=bufs["ema"][1] if ema else None,
                            ema_decay=DECAY if ema else 0.0, **kw)
    torch.cuda.synchronize()
    return bufs, gbufs


def test_lamb_edge_shapes_match_fp64_and_leave_gaps_and_guard_zones_alone(ops):
    sizes, offs, total, scales, wds, tensors, grads = _case(True)
    assert sizes[-1] == 256 * 4096 + 1                                          # 257 items: more than a workgroup has threads
    r64, bars, want_e = _lamb_reference()
    assert min(r64.trust) < 0.9 and max(r64.trust) > 1.1 and r64.trust.count(1.0) >= 15       # both sides of 1, and wd = 0 tensors
    coef = torch.tensor([COEF]).cuda()
    bufs, gbufs = _lamb_run(ops, sizes, offs, total, list(zip(scales, wds)), tensors, grads, grad_scale=GSCALE, clip_coef=coef)
    rows, failed = [], []
    for k, (o, n) in enumerate(zip(offs, sizes)):
        ep, em, ev = (relerr(bufs[name][1][o:o + n], want[k]) for name, want in (("p", r64.p), ("m", r64.m), ("v", r64.v)))
        ee = relerr(bufs["ema"][1][o:o + n], want_e[k])
        base, bar = bars[k]
        rows.append(f"{k} {n} {scales[k]:.6g} {wds[k]:g} {r64.trust[k]:.6e} {base:.6e} {bar:.6e} {ep:.6e} {ee:.6e} {em:.6e} {ev:.6e}")
        if not (ep < bar and ee < bar and em < BAR and ev < BAR):
            failed.append(rows[-1])
    head = ["# mv_lamb_table on the edge arena + one tensor of 256 * 4096 + 1 elements, three steps: per tensor, max |got - fp64| /",
            "# max |fp64|.  baseline = torch's own fp32 evaluation of the same formulas against fp64 (tests/optim_family_ref.py);",
            f"# bar_p = max({BAR:g}, 8 x baseline) holds p and the EMA, {BAR:g} holds m and v.  trust = the fp64 trust ratio of step 3.",
            "# tensor elements lr_scale wd trust baseline bar_p p ema m v"]
    text = "\n".join(head + rows) + "\n"
    print(text)
    out = os.environ.get("MV_OPTIM_FAMILY_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            f.write(text)
    assert not failed, failed
    gaps = gap_mask(offs, sizes, total).cuda()
    for name, (buf, arr) in bufs.items():
        assert _canaries_intact(buf), name
        assert bool((arr[gaps] == 0).all()), name
    for gbuf, before in gbufs:
        assert torch.equal(gbuf, before)
    again, _ = _lamb_run(ops, sizes, offs, total, list(zip(scales, wds)), tensors, grads, grad_scale=GSCALE, clip_coef=coef)
    for name in bufs:
        assert torch.equal(bufs[name][0], again[name][0]), name                 # two runs from the same state, the same bits
    # the same tensor stepped ALONE in an arena: the same bits (70 001 elements: 18 items; the large one: 257)
    for k in (10, len(sizes) - 1):
        n, o = sizes[k], offs[k]
        alone, _ = _lamb_run(ops, [n], [0], (n + 7) & ~7, [(scales[k], wds[k])], [tensors[k]], [[gs[k]] for gs in grads],
                             grad_scale=GSCALE, clip_coef=coef)
        for name in bufs:
            assert torch.equal(alone[name][1][:n], bufs[name][1][o:o + n]), (k, name)


# ---------------------------------------------------------------- LAMB's branches, each on a tiny arena
def _tiny(ops, sizes, pairs, tensors, grads, lr):
    offs, total = arena_offsets(sizes)
    items, seg_scale, seg_wd, item_tensor, tensor_range = _tables(sizes, offs, pairs)
    p, m, v = flat(tensors, offs, total).cuda(), torch.zeros(total).cuda(), torch.zeros(total).cuda()
    ops.lamb_table_step(p, flat(grads, offs, total).cuda(), m, v, items, item_tensor, tensor_range, seg_scale, seg_wd,
                        ops.lamb_workspace(items[0].numel(), p.device), lr=lr, beta1=0.9, beta2=0.999, eps=1e-6, step=1)
    torch.cuda.synchronize()
    ref = LambReference(tensors, [s for s, _ in pairs], [w for _, w in pairs])
    ref.step(lr, grads)
    return [p[o:o + n].cpu() for o, n in zip(offs, sizes)], [m[o:o + n].cpu() for o, n in zip(offs, sizes)], ref


def test_lamb_all_zero_tensor_steps_with_trust_one(ops):
    sizes = [5000, 7]
    tensors, grads = [torch.zeros(n) for n in sizes], [torch.randn(n, generator=g(31 + n)) for n in sizes]
    p, _, ref = _tiny(ops, sizes, [(1.0, 0.05), (0.5, 0.05)], tensors, grads, 1e-2)
    assert ref.trust == [1.0, 1.0]                                              # ||p|| = 0
    for got, want in zip(p, ref.p):
        assert bool(torch.isfinite(got).all()) and bool((got != 0).all())
        assert relerr(got, want) < BAR


def test_lamb_zero_gradient_zero_state_no_decay_leaves_p_unchanged(ops):
    sizes = [5000, 3]
    tensors, grads = [torch.randn(n, generator=g(41 + n)) for n in sizes], [torch.zeros(n) for n in sizes]
    p, m, ref = _tiny(ops, sizes, [(1.0, 0.0), (1.0, 0.0)], tensors, grads, 1e-2)
    assert ref.trust == [1.0, 1.0]
    for got, before, mom in zip(p, tensors, m):
        assert torch.equal(got, before) and not bool(mom.any())                 # u = 0 / (0 + eps) = 0: no NaN, p bit for bit


def test_lamb_trust_applies_to_decayed_tensors_only(ops):
    """Two copies of one tensor with ||p|| / ||u|| far from 1: the copy with wd = 0 steps by lr * u (trust stays 1, timm's rule); the
    copy whose wd is not 0 -- but so small that wd * p vanishes under u's last bit, so u is the same -- steps ||p|| / ||u|| times as far."""
    n, lr, tiny_wd = 5000, 1e-2, 1e-30
    t, gr = torch.randn(n, generator=g(51)) * 4, torch.randn(n, generator=g(52))
    (p0, pw), _, ref = _tiny(ops, [n, n], [(1.0, 0.0), (1.0, tiny_wd)], [t, t.clone()], [gr, gr.clone()], lr)
    trust = ref.trust[1]
    assert ref.trust[0] == 1.0 and 3.0 < trust < 5.0
    assert relerr(p0, ref.p[0]) < BAR and relerr(pw, ref.p[1]) < BAR
    d0, dw = (t - p0).double(), (t - pw).double()
    assert 0.9 * lr < float(d0.abs().max()) < 1.1 * lr                          # the first step's u is g / (|g| + eps'): +-1
    # each of p0, pw is one fp32 rounding of its exact value (half an ulp of max |p| < 32: 2^-20); the rate lr * trust adds one more
    # rounding of the step itself, relative 2^-23
    tol = (1.0 + trust) * 2.0 ** -20 + trust * lr * 2.0 ** -22
    assert float((dw - trust * d0).abs().max()) < tol


# ---------------------------------------------------------------- equivalence to the existing kernel
def test_lamb_with_every_trust_one_takes_the_adamw_table_step(ops):
    """All wd = 0 (every trust ratio 1), no clip: from the same state LAMB's step is AdamW's.  This ties the moment arithmetic to the
    kernel that is already held to torch."""
    sizes, offs, total, scales, _, tensors, grads = _case(False)
    items, seg_scale, seg_wd, item_tensor, tensor_range = _tables(sizes, offs, [(s, 0.0) for s in scales])
    ws = ops.lamb_workspace(items[0].numel(), torch.device("cuda"))
    pa, ma, va = flat(tensors, offs, total).cuda(), torch.zeros(total).cuda(), torch.zeros(total).cuda()
    for s in range(3):
        gr = flat(grads[s], offs, total).cuda()
        pl, ml, vl = pa.clone(), ma.clone(), va.clone()                         # the same state before every step
        kw = dict(lr=LRS[s], beta1=0.9, beta2=0.999, eps=1e-8, step=s + 1, grad_scale=GSCALE)
        ops.adamw_table_step(pa, gr, ma, va, items, seg_scale, seg_wd, **kw)
        ops.lamb_table_step(pl, gr, ml, vl, items, item_tensor, tensor_range, seg_scale, seg_wd, ws, **kw)
        torch.cuda.synchronize()
        for k, (o, n) in enumerate(zip(offs, sizes)):
            for name, got, want in (("p", pl, pa), ("m", ml, ma), ("v", vl, va)):
                assert relerr(got[o:o + n], want[o:o + n]) < BAR, (s, k, name)
    assert not torch.equal(pa, flat(tensors, offs, total).cuda())


# ---------------------------------------------------------------- graph capture
RECIPE = dict(layer_decay=0.75, no_weight_decay=["pos_embedding", "cls_token"], ema_decay=0.99)


def _state(opt):
    return {n: getattr(opt, n) for n in ("exp_avg", "exp_avg_sq", "momentum_buffer") if getattr(opt, n, None) is not None}


@pytest.mark.parametrize("kind", ["sgd", "lamb"])
def test_graphed_step_equals_eager_step(kind):
    """tests/test_optim_table_gpu.py's capture test on TableSGD and TableLamb, each with layer decay, exempt names, the EMA and
    clip_grad: replays with a learning-rate change in between give, bit for bit, the parameters, state and EMA of the eager steps."""
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.graph import GraphedTrainStep
    from myrtle_vision.utils.optim import ParamArena, TableLamb, TableSGD
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
        arena = ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names())
        if kind == "sgd":
            opt = TableSGD(arena, lr=1e-3, momentum=0.9, nesterov=True, weight_decay=0.05, **RECIPE)
        else:
            opt = TableLamb(arena, lr=1e-3, weight_decay=0.05, **RECIPE)
        opt.max_grad_norm = 0.5                                              # clip_grad: below LAMB's own 1.0, so the step clips to it
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
    sg, se = _state(opt_g), _state(opt_e)
    assert list(sg) == (["momentum_buffer"] if kind == "sgd" else ["exp_avg", "exp_avg_sq"])
    for name in sg:
        assert torch.equal(sg[name], se[name]) and bool(sg[name].any()), name
    assert torch.equal(opt_g.ema, opt_e.ema) and not torch.equal(opt_g.ema, opt_g.arena.flat_param)
    assert float(opt_e.last_grad_norm[1]) < 1.0                                  # the clip engaged
    vit_g.eval(), vit_e.eval()
    with torch.no_grad(), opt_g.ema_weights(), opt_e.ema_weights():
        assert torch.equal(vit_g(batches[0][0]), vit_e(batches[0][0]))


# ---------------------------------------------------------------- the training loop
@pytest.mark.parametrize("name", ["lamb", "sgd"])
def test_train_worker_with_the_optimizer_key(name, tmp_path, capsys):
    """Two iterations of the segmentation loop on the synthetic set, as tests/test_optim_table_gpu.py runs them for the three keys (one
    validation instead of two: the EMA's logging is that test's subject): the run finishes with finite losses, its checkpoints carry
    the optimizer's kind and load back, also with "use_ema"."""
    from myrtle_vision.datasets.synthetic import make_dlrsd
    from myrtle_vision.engine import evaluate, train_worker
    cfg = json.load(open(os.path.join(ROOT, "segmentation", "train_configs", "seg_tiny.json")))
    data = json.load(open(os.path.join(ROOT, "segmentation", "data_configs", "data_config.json")))
    data["dataset_path"] = make_dlrsd(str(tmp_path / "DLRSD_dataset"), count=32)
    cfg["data_config_path"] = str(tmp_path / "data_config.json")
    json.dump(data, open(cfg["data_config_path"], "w"))
    out_dir = str(tmp_path / "ckpt")
    cfg["train_config"].update(output_directory=out_dir, epochs=1, local_batch_size=8, global_batch_size=8, iters_per_checkpoint=1,
                               iters_per_val=1000, distributed=False, pretrained_backbone=None, tensorboard_dir=str(tmp_path / "runs"),
                               optimizer=name, layer_decay=0.75, no_weight_decay=["pos_embedding", "cls_token"], model_ema_decay=0.5)
    cfg["vit_config"]["depth"] = 2
    iters = train_worker(0, 1, copy.deepcopy(cfg), "segmentation")
    out = capsys.readouterr().out
    assert iters == 2 and "nan" not in out.lower()
    assert "val_loss_ema" in out
    ck = torch.load(os.path.join(out_dir, "vit_000001"), map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "iteration", "model_ema"}
    assert ck["optimizer"]["kind"] == name and ck["optimizer"]["layer_decay"] == 0.75
    field = "exp_avg" if name == "lamb" else "momentum_buffer"
    assert all(bool(torch.isfinite(e[field]).all()) for e in ck["optimizer"]["state"].values()) and ck["optimizer"]["state"]
    w = "transformer.layers.0.0.fn.fn.to_qkv.weight"
    assert bool(torch.isfinite(ck["model"][w]).all()) and not torch.equal(ck["model_ema"][w], ck["model"][w])
    ck0 = torch.load(os.path.join(out_dir, "vit_000000"), map_location="cpu", weights_only=False)
    assert not torch.equal(ck0["model"][w], ck["model"][w])                      # the step moved the weights
    # the optimizer part loads back into an optimizer of its kind, with its state, its count and the EMA
    from myrtle_vision.utils.models import get_models, get_optimizer_args, load_checkpoint
    from myrtle_vision.utils.optim import create_optimizer, create_scheduler
    vit = get_models(cfg)[0].cuda()
    args = get_optimizer_args(cfg["train_config"])
    opt = create_optimizer(args, vit)
    assert load_checkpoint(vit, opt, create_scheduler(args, opt)[0], os.path.join(out_dir, "vit_000001")) == ck["iteration"]
    assert opt.kind == name and opt.step_count == 1 and opt.ema_loaded
    state = opt.exp_avg if name == "lamb" else opt.momentum_buffer
    assert bool(state.any()) and bool(torch.isfinite(state).all())
    cfg2 = copy.deepcopy(cfg)
    cfg2["train_config"]["checkpoint_path"] = os.path.join(out_dir, "vit_000001")
    cfg2["use_ema"] = True
    res = evaluate(cfg2, "segmentation")
    assert 0.0 <= res["accuracy"] <= 1.0
