"""GPU: DeiT distillation -- ``mv_distill_loss`` against the fp64 oracle of tests/distill_ref.py at 8 x torch's own fp32 error
(computed when the tests run) and its exact properties; the token append and the head's ``row`` argument bit for bit; the
``DistillWrapper`` against a composition of the same package blocks with torch ops in place of the new parts; the training loop
end to end."""
import copy
import json
import os

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402
import distill_ref as R  # noqa: E402

DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _all_plus_zero(t):
    """Every element is +0.0: no set bit anywhere, the sign bit included."""
    return bool((_bits(t) == 0).all())


# ================================================================== the loss kernel against the fp64 oracle
@pytest.mark.parametrize("C", R.CLASSES)
@pytest.mark.parametrize("B", R.BATCHES)
def test_distill_loss_meets_eight_times_torchs_fp32_error(B, C):
    """Every (T, alpha, mode, labelling) of one (B, C): 24 launches.  The bound is 8 x the largest error of torch's fp32 evaluation
    over ALL cases (distill_ref.baselines, computed once per session); figures: profiles/distill_parity.txt."""
    assert R.teacher_gap(R.inputs(B, C)[2]) > 0                  # fp32 and fp64 agree on the teacher's arg-max: no case is skipped
    base = R.baselines()
    got = R.kernel_errors(B, C, DEV)
    for k in R.QUANTITIES:
        print(f"B={B} C={C} {k}: kernel {got[k]:.3e}  baseline {base[k]:.3e}  bound {R.FACTOR * base[k]:.3e}")
    for k in R.QUANTITIES:
        assert got[k] <= R.FACTOR * base[k], (k, got[k], base[k])


# ================================================================== exact properties of the loss kernel
def _run(B, C, T=3.0, alpha=0.5, mode="soft", labelling=R.LABELLINGS[0], labels=None):
    from myrtle_vision.hip import ops
    s, d, t, y = (v.to(DEV) for v in R.inputs(B, C))
    y = y if labels is None else labels.to(DEV)
    return ops.distill_loss(s, d, t, y, T, alpha, mode, *labelling, want_grad=True, want_argmax=True), (s, d, t, y)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("B,C", [(7, 45), (64, 1001)])
def test_zero_weight_gives_zero_bits_and_argmax_is_torchs(B, C, mode):
    for labelling in R.LABELLINGS:
        (loss, ds, dd, am, _), (s, _, _, _) = _run(B, C, alpha=1.0, mode=mode, labelling=labelling)
        assert _all_plus_zero(dd) and float(ds.abs().max()) > 0                        # +0 everywhere, never -0
        assert float(loss[0]) == float(loss[1])
        assert torch.equal(am, s.argmax(dim=1)) and am.dtype == torch.int64
        (loss, ds, dd, am, _), _ = _run(B, C, alpha=0.0, mode=mode, labelling=labelling)
        assert _all_plus_zero(ds) and float(dd.abs().max()) > 0
        assert float(loss[0]) == float(loss[2])
        assert torch.equal(am, s.argmax(dim=1))


def test_argmax_takes_the_first_of_equal_logits():
    from myrtle_vision.hip import ops
    s, d, t, y = (v.to(DEV).clone() for v in R.inputs(7, 1001))
    s[:, 900] = s[:, 70] = s.max() + 1.0                         # a tie across two lanes' strides
    am = ops.distill_loss(s, d, t, y, want_argmax=True)[3]
    assert torch.equal(am, torch.full((7,), 70, device=DEV)) and torch.equal(am, s.argmax(dim=1))


@pytest.mark.parametrize("mode", R.MODES)
def test_two_runs_give_identical_bits_and_the_ce_is_cross_entropy_softs(mode):
    from myrtle_vision.hip import ops
    for labelling in R.LABELLINGS:
        (a, (s, d, t, y)), (b, _) = _run(64, 1000, mode=mode, labelling=labelling), _run(64, 1000, mode=mode, labelling=labelling)
        for u, v in zip(a, b):
            assert torch.equal(_bits(u) if u.dtype == torch.float32 else u, _bits(v) if v.dtype == torch.float32 else v)
        # CE_i is the per-sample value of mv_cross_entropy_soft, and its mean the same fixed-order mean
        ce, _, _, per_sample = ops.cross_entropy_soft(s, y, *labelling)
        assert torch.equal(_bits(a[4][0]), _bits(per_sample)) and torch.equal(_bits(a[0][1:2]), _bits(ce))


@pytest.mark.parametrize("mode", R.MODES)
def test_out_of_range_label_poisons_its_sample_only(mode):
    B, C = 7, 45
    y = R.inputs(B, C)[3].clone()
    for bad in (C, -1, 1 << 40):
        yb = y.clone()
        yb[2] = bad
        (good, _), (got, _) = _run(B, C, mode=mode), _run(B, C, mode=mode, labels=yb)
        loss, ds, dd, am, per = got
        assert bool(torch.isnan(loss[0])) and bool(torch.isnan(loss[1])) and bool(torch.isnan(per[0, 2]))
        assert _all_plus_zero(ds[2])
        keep = [i for i in range(B) if i != 2]
        assert torch.equal(_bits(ds[keep]), _bits(good[1][keep])) and torch.equal(_bits(per[0, keep]), _bits(good[4][0, keep]))
        # the distillation term does not look at the label
        assert torch.equal(_bits(dd), _bits(good[2])) and torch.equal(_bits(per[1]), _bits(good[4][1])) and torch.equal(am, good[3])
    # the partner's label poisons too, under pair_flip (sample i reads the label of B - 1 - i)
    yb = y.clone()
    yb[0] = C
    loss, ds, _, _, per = _run(B, C, mode=mode, labelling=R.LABELLINGS[1], labels=yb)[0]
    assert torch.isnan(per[0]).tolist() == [True] + [False] * (B - 2) + [True] and bool(torch.isnan(loss[0]))
    assert _all_plus_zero(ds[[0, B - 1]]) and float(ds[1:B - 1].abs().max()) > 0


GUARD = 256


def _guarded(src=None, numel=None, dtype=torch.float32, canary=None):
    """A buffer with ``GUARD`` canary elements in front of and behind the payload -> (payload view, whole buffer)."""
    n = src.numel() if src is not None else numel
    dtype = src.dtype if src is not None else dtype
    canary = canary if canary is not None else (-777.0 if dtype == torch.float32 else -777)
    whole = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device=DEV)
    body = whole[GUARD:GUARD + n]
    if src is not None:
        body.copy_(src.reshape(-1))
    return body, whole, canary


@pytest.mark.parametrize("mode", [0, 1], ids=R.MODES)
@pytest.mark.parametrize("B,C", [(1, 2), (7, 65), (64, 1001)])
def test_guard_zones_keep_their_canary_and_the_teacher_is_only_read(B, C, mode):
    from myrtle_vision.hip import lib
    s, d, t, y = R.inputs(B, C)
    ins = [_guarded(v.to(DEV)) for v in (s, d, t, y)]
    outs = [_guarded(numel=3), _guarded(numel=2 * B), _guarded(numel=B * C), _guarded(numel=B * C),
            _guarded(numel=B, dtype=torch.int64)]
    before = [w.clone() for _, w, _ in ins]
    rc = lib.lib().mv_distill_loss(*[b.data_ptr() for b, _, _ in ins], *[b.data_ptr() for b, _, _ in outs], B, C, mode, 3.0, 0.5,
                                   0.3, 0.1, 1, 1.0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for (_, whole, _), was in zip(ins, before):                  # inputs, the teacher among them: untouched, guards and payload
        assert torch.equal(whole, was)
    for body, whole, canary in outs:
        assert bool((whole[:GUARD] == canary).all()) and bool((whole[-GUARD:] == canary).all())
        assert not bool((body == canary).any())                  # and every element of the payload was written
    ref = R.oracle(s.numpy(), d.numpy(), t.numpy(), y.numpy(), 3.0, 0.5, R.MODES[mode], 0.3, 0.1, True)
    assert abs(float(outs[0][0][0]) - ref["loss"]) < 1e-4 * abs(ref["loss"])


# ================================================================== append
@pytest.mark.parametrize("D", [128, 192])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_token_append_is_cat_and_its_backward_the_slice_and_the_ordered_sum(B, D):
    from myrtle_vision.hip import functional as F
    T0 = 5
    g = torch.Generator().manual_seed(B * 1000 + D)
    x = torch.randn(B, T0, D, generator=g).to(DEV).requires_grad_(True)
    tok = torch.randn(1, 1, D, generator=g)
    tok[0, 0, :4] = torch.tensor([0.0, -0.0, 1e-45, -1e-45])      # both zeros and the denormals keep their bits
    tok = tok.to(DEV).requires_grad_(True)
    out = F.token_append(x, tok)
    assert out.shape == (B, T0 + 1, D) and out.dtype == torch.float32
    assert torch.equal(_bits(out), _bits(torch.cat((x, tok.expand(B, 1, D)), dim=1).detach()))
    dout = torch.randn(B, T0 + 1, D, generator=g).to(DEV)
    out.backward(dout)
    assert torch.equal(_bits(x.grad), _bits(dout[:, :T0]))
    last = dout[:, T0].double().cpu()
    bound = (B - 1) * 2.0 ** -24 * last.abs().sum(dim=0)         # a fixed-order fp32 sum of B terms
    assert tok.grad.shape == (1, 1, D)
    assert bool(((tok.grad.view(D).double().cpu() - last.sum(dim=0)).abs() <= bound).all())
    if B == 1:
        assert torch.equal(_bits(tok.grad.view(D)), _bits(dout[0, T0]))
    # the same bits on a second pass (batch order, no atomics)
    x2, tok2 = x.detach().clone().requires_grad_(True), tok.detach().clone().requires_grad_(True)
    F.token_append(x2, tok2).backward(dout)
    assert torch.equal(_bits(tok2.grad), _bits(tok.grad))


# ================================================================== head row
def _head(prec, row, x, params, dl):
    from myrtle_vision.hip import functional as F
    x = x.detach().clone().requires_grad_(True)
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    logits = F.cls_head(x, *ps, prec) if row is None else F.cls_head(x, *ps, prec, row=row)
    logits.backward(dl)
    return [logits.detach(), x.grad] + [p.grad for p in ps]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_cls_head_row_moves_the_base_pointer_only(prec):
    B, T, D, C = 4, 27, 128, 10
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, D, generator=g).to(DEV)
    params = [v.to(DEV) for v in (1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g),
                                  0.1 * torch.randn(C, D, generator=g), 0.1 * torch.randn(C, generator=g))]
    dl = torch.randn(B, C, generator=g).to(DEV)
    default, zero = _head(prec, None, x, params, dl), _head(prec, 0, x, params, dl)
    for a, b in zip(default, zero):
        assert torch.equal(_bits(a), _bits(b))
    last = _head(prec, T - 1, x, params, dl)
    rolled = _head(prec, None, torch.roll(x, 1, dims=1), params, dl)          # row T-1 becomes row 0
    rolled[1] = torch.roll(rolled[1], -1, dims=1)
    for a, b in zip(last, rolled):
        assert torch.equal(_bits(a), _bits(b))
    assert float(last[1][:, T - 1].abs().max()) > 0 and _all_plus_zero(last[1][:, :T - 1])
    assert not torch.equal(last[0], default[0])
    with pytest.raises(ValueError, match="row"):
        _head(prec, T, x, params, dl)


# ================================================================== model level
def _wrapper(prec, image=80, dim=128, heads=2, depth=2, classes=10, mode="soft", **student_kw):
    from myrtle_vision.models.distill import DistillableViT, DistillWrapper
    from myrtle_vision.models.vit import ViT
    kw = dict(decoder="classification", image_size=image, patch_size=16, num_classes=classes, dim=dim, heads=heads, mlp_dim=2 * dim,
              precision=prec)
    torch.manual_seed(7)
    teacher = ViT(depth=1, **kw)
    student = DistillableViT(depth=depth, **kw, **student_kw)
    w = DistillWrapper(teacher=teacher, student=student, temperature=3.0, alpha=0.5, distillation_type=mode)
    with torch.no_grad():                                        # pos_embedding is [1, 197, D] whatever the image: keep it small
        for p in w.parameters():
            if p.dim() == 3:
                p.mul_(0.2)
    return w.to(DEV).train()


def _composition(w, img, labels, T, alpha, mode):
    """The wrapper's computation from the same package blocks, with torch ops in place of the new parts: ``torch.cat`` for the append,
    fp32 ``layer_norm`` / ``linear`` for the distillation head, ``cross_entropy`` + ``kl_div`` for the loss."""
    from myrtle_vision.hip import functional as F
    from myrtle_vision.hip import ops
    st = w.student
    B = img.shape[0]
    with torch.no_grad():
        tl = w.teacher(img).float()
    F.chain_reset()
    g = img.shape[-1] // st.patch_size
    with ops.segments(ops.prec_segments(st.precision)):
        x = F.patch_embed(img, st.patch_to_embedding.weight, st.patch_to_embedding.bias, st.cls_token, st._pos_embedding(g, g),
                          st.patch_size, st.precision)
        x = torch.cat((x.float(), w.distillation_token.expand(B, 1, -1)), dim=1)
        x = st.transformer(st.dropout(x))
        logits = st.decoder(x)
    norm, lin = w.distill_mlp
    dl = TF.linear(TF.layer_norm(x[:, -1].float(), (x.shape[-1],), norm.weight, norm.bias, norm.eps), lin.weight, lin.bias)
    ce = TF.cross_entropy(logits, labels)
    if mode == "soft":
        kd = TF.kl_div(TF.log_softmax(dl / T, dim=-1), TF.softmax(tl / T, dim=-1).detach(), reduction="batchmean") * T ** 2
    else:
        kd = TF.cross_entropy(dl, tl.argmax(dim=1))
    return ce * alpha + kd * (1 - alpha)


def _compare(prec, mode="soft", B=4, **shape):
    loss_tol, grad_tol = (1e-3, 1e-3) if prec == "fp32" else (1.5e-2, 2e-2)              # the project's per-precision bars
    w = _wrapper(prec, mode=mode, **shape)
    ref = copy.deepcopy(w)
    g = torch.Generator().manual_seed(3)
    size = shape.get("image", 80)
    img = torch.randn(B, 3, size, size, generator=g).to(DEV)
    labels = torch.randint(0, 10, (B,), generator=g).to(DEV)
    loss, am = w(img, labels, return_argmax=True)
    loss.backward()
    want = _composition(ref, img, labels, 3.0, 0.5, mode)
    want.backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    print(f"{prec} {mode}: loss {float(loss):.6f} composition {float(want):.6f}")
    assert abs(float(loss) - float(want)) <= loss_tol * abs(float(want))
    with torch.no_grad():                                        # the kernel's arg-max is that of the class logits of this very pass
        assert torch.equal(am, w.student(img, w.distillation_token)[0].argmax(dim=1))
    names = []
    for (n, p), (_, q) in zip(w.named_parameters(), ref.named_parameters()):
        if n.startswith("teacher."):
            assert p.grad is None and not p.requires_grad, n
            continue
        if q.grad is None:
            assert p.grad is None and n in w.unused_parameter_names(), n
            continue
        err = float((p.grad.float() - q.grad.float()).norm() / q.grad.float().norm().clamp_min(1e-30))
        assert err <= grad_tol, (n, err)
        names.append(n)
    assert {"distillation_token", "distill_mlp.0.weight", "distill_mlp.1.bias", "student.cls_token"} <= set(names)
    assert float(w.distillation_token.grad.abs().max()) > 0
    return w, img


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_wrapper_matches_the_composition(prec, mode):
    """image 80 / patch 16: 27 tokens with both extra ones; dim 128, heads 2, depth 2, B 4, 10 classes, a depth-1 ViT teacher."""
    _compare(prec, mode)


def test_routing_case_at_the_real_sequence_length():
    """image 224, dim 192, heads 3, depth 1, B 2, bf16: N = 198, one past the 197 the attention kernels are tuned for."""
    w, img = _compare("bf16", B=2, image=224, dim=192, heads=3, depth=1)
    with torch.no_grad():
        logits, tokens = w.student(img, w.distillation_token)
    assert logits.shape == (2, 10) and tokens.shape == (2, 192) and logits.dtype == tokens.dtype == torch.float32
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(tokens).all())


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_without_a_token_it_is_the_plain_vit_and_pruning_is_ignored_with_one(prec):
    from myrtle_vision.models.distill import DistillableViT
    from myrtle_vision.models.vit import ViT
    w = _wrapper(prec).eval()
    st = w.student
    img = torch.randn(4, 3, 80, 80, generator=torch.Generator().manual_seed(5)).to(DEV)
    plain = ViT(**st.kwargs).to(DEV).eval()
    plain.load_state_dict(st.state_dict())
    pruned = DistillableViT(**st.kwargs, prune_dead_tokens=True).to(DEV).eval()
    pruned.load_state_dict(st.state_dict())
    assert pruned.transformer.cls_only_tail and not st.transformer.cls_only_tail
    with torch.no_grad():
        assert torch.equal(_bits(st(img)), _bits(plain(img)))
        logits, tokens = st(img, w.distillation_token)
        logits_p, tokens_p = pruned(img, w.distillation_token)
        assert torch.equal(_bits(logits), _bits(logits_p)) and torch.equal(_bits(tokens), _bits(tokens_p))
        assert pruned.transformer.cls_only_tail                  # put back
        assert torch.equal(_bits(pruned(img)), _bits(plain(img)))  # and still the plain model's logits without a token
        assert not torch.equal(logits, st(img))                  # the extra token is seen by the attention


# ================================================================== end to end
def _config(tmp_path):
    """deit_tiny.json cut down as tests/test_train_gpu.py::_config does; the teacher is a depth-2 ViT-S on the host file system."""
    from myrtle_vision.datasets.synthetic import make_resisc45
    from myrtle_vision.models.vit import ViT
    cfg = json.load(open(os.path.join(ROOT, "classification", "train_configs", "deit_tiny.json")))
    small = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_small.json")))["vit_config"]
    data = json.load(open(os.path.join(ROOT, "classification", "data_configs", "data_config.json")))
    data["dataset_path"] = make_resisc45(str(tmp_path / "NWPU-RESISC45"), classes=45, per_class=2)
    dpath = str(tmp_path / "data_config.json")
    json.dump(data, open(dpath, "w"))
    cfg["data_config_path"] = dpath
    cfg["train_config"].update(output_directory=str(tmp_path / "ckpt"), epochs=1, local_batch_size=8, global_batch_size=8,
                               iters_per_checkpoint=2, iters_per_val=2, distributed=False, pretrained_backbone=None)
    cfg["vit_config"]["depth"] = 2
    tv = dict(small, depth=2)
    torch.manual_seed(1)
    teacher = ViT(decoder="classification", image_size=224, patch_size=16, num_classes=45, dim=tv["embed_dim"], depth=2,
                  heads=tv["heads"], mlp_dim=tv["mlp_dim"])
    path = str(tmp_path / "teacher.pt")
    torch.save(teacher.state_dict(), path)
    cfg["distiller_config"].update(teacher_vit_config=tv, teacher_weights_path=path)
    return cfg


def _losses(out):
    return [float(l.split("loss=")[1].split()[0]) for l in out.splitlines() if l.startswith("Iteration")]


def test_train_loop_distils_checkpoints_resumes_and_evaluates(tmp_path, capsys):
    from myrtle_vision import engine
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.utils import parse_config
    cfg = _config(tmp_path)
    iters = engine.train_worker(0, 1, copy.deepcopy(cfg), "classification")
    out = capsys.readouterr().out
    losses = _losses(out)
    assert iters >= 2 and len(losses) == iters and all(l == l and l < 50 for l in losses) and "nan" not in out.lower()
    d = cfg["train_config"]["output_directory"]
    ck0 = torch.load(os.path.join(d, "vit_000000"), map_location="cpu", weights_only=False)
    ck = torch.load(os.path.join(d, "vit_000002"), map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "iteration", "distiller"} and ck["iteration"] == 2
    v = cfg["vit_config"]
    plain = ViT(decoder="classification", image_size=224, patch_size=16, num_classes=45, dim=v["embed_dim"], depth=2,
                heads=v["heads"], mlp_dim=v["mlp_dim"])
    assert plain.load_state_dict(ck["model"], strict=True).missing_keys == []
    assert set(ck["distiller"]) == {"distillation_token", "distill_mlp.0.weight", "distill_mlp.0.bias", "distill_mlp.1.weight",
                                    "distill_mlp.1.bias"}
    for k in ("distillation_token", "distill_mlp.1.weight"):     # two optimizer steps moved the token and the head
        assert not torch.equal(ck["distiller"][k], ck0["distiller"][k]), k
    # resume: model, optimizer and the distiller's own parameters come back bit for bit
    cfg2 = copy.deepcopy(cfg)
    cfg2["train_config"]["checkpoint_path"] = os.path.join(d, "vit_000002")
    device = torch.device("cuda", 0)
    vit, optimizer, sched, args, distiller = engine._model_and_optimizer(0, cfg2, parse_config(cfg2["data_config_path"]), device)
    assert not any(n.startswith("teacher.") for n in optimizer.arena.names)
    assert {"distillation_token", "distill_mlp.1.weight", "student.cls_token"} <= set(optimizer.arena.names)
    iteration, _, _ = engine._resume(cfg2["train_config"], vit, optimizer, sched, args.clip_grad, 1, 8, 90, 1, distiller=distiller)
    assert iteration == 2
    for k, val in ck["distiller"].items():
        assert torch.equal(distiller.state_dict()[k].cpu(), val), k
    for k, val in ck["model"].items():
        assert torch.equal(vit.state_dict()[k].cpu(), val), k
    assert "WARNING" not in capsys.readouterr().out
    # evaluation needs the student alone: no teacher file
    os.remove(cfg["distiller_config"]["teacher_weights_path"])
    res = engine.evaluate(cfg2, "classification")
    assert 0.0 <= res["accuracy"] <= 1.0


def test_train_loop_distils_under_label_smoothing_and_mixup(tmp_path, capsys):
    from myrtle_vision import engine
    cfg = _config(tmp_path)
    cfg["train_config"].update(label_smoothing=0.1, mixup_alpha=0.8, iters_per_checkpoint=1000, iters_per_val=1000)
    cfg["vit_config"]["drop_path_rate"] = 0.1
    iters = engine.train_worker(0, 1, copy.deepcopy(cfg), "classification")
    out = capsys.readouterr().out
    losses = _losses(out)
    assert iters >= 2 and len(losses) == iters and all(l == l and l < 50 for l in losses) and "nan" not in out.lower()
