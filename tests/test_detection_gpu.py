"""YOLOS detection on the GPU: model goldens from the reference (tests/golden/micro_det, base_det), every kernel of
csrc/detection.hip alone against an fp64 restatement (tests/detection_ref.py), the opt-in live detection tokens.

Kernel tolerances are not fixed in advance: profiles/detection_parity.txt holds, per quantity, the error of torch's own fp32 CPU
evaluation of the same formulas against fp64 on the same inputs (baseline) and 8 x that (bound); TABLE below is that file.
Kernel outputs sit in the middle of larger allocations filled with a sentinel (guard zones, as tests/test_attention_short.py).

MV_TEST_REPORT=<file>: every check appends the value it measured.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT, load_golden  # noqa: E402
from oracle.detinit import det_images, det_param, summarize  # noqa: E402

import detection_ref as ref  # noqa: E402

TABLE = ref.read_parity_table(os.path.join(ROOT, "profiles", "detection_parity.txt"))
EXACT = ("fp32", "bf16x3")
TOL_OUT = {"fp32": 1e-3, "bf16x3": 1e-3, "bf16": 1.5e-2}        # of max |value| (tests/test_vit_parity.py)
# gradient summaries: bf16's are norms + 16 sampled values against the tensor's abs-max, the noisier statistic held to 3e-2 by
# tests/test_vit_parity.py::test_bf16_matches_reference_within_bf16_envelope (the 2e-2 there is the full-tensor relative L2)
TOL_GRAD = {"fp32": 1e-3, "bf16x3": 1e-3, "bf16": 3e-2}
SENTINEL = 0xA5


def report(tag, value):
    path = os.environ.get("MV_TEST_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"{tag} {value:.3e}\n")


def within(q, err, tag=""):
    base, bound = TABLE[q]
    report(f"detection-kernel {q} {tag} (baseline {base:.3e}, bound {bound:.3e})", err)
    print(f"{q} {tag}: err {err:.3e} baseline {base:.3e} bound {bound:.3e}")
    assert err <= bound, (q, tag, err, bound)


# ------------------------------------------------------------------------------------------------------------ guard zones
class Guarded:
    """Output tensors in the middle of sentinel-filled allocations, bodies prefilled with NaN / a poison integer."""

    def __init__(self):
        self.items = []

    def out(self, shape, dtype=torch.float32):
        n = int(np.prod(shape)) if len(shape) else 1
        es = torch.empty(0, dtype=dtype).element_size()
        guard = 4096
        raw = torch.full(((n * es + 15) // 16 * 16 + 2 * guard,), SENTINEL, dtype=torch.uint8, device="cuda")
        body = raw[guard:guard + n * es].view(dtype).view(shape)
        if dtype.is_floating_point:
            body.fill_(float("nan"))
        else:
            body.fill_(-(1 << 20))
        self.items.append((raw, guard, n * es))
        return body

    def check(self):
        torch.cuda.synchronize()
        for raw, g, nb in self.items:
            assert bool((raw[:g] == SENTINEL).all()) and bool((raw[g + nb:] == SENTINEL).all()), "a guard byte changed"


def pack(targets):
    from myrtle_vision.models.matcher import PackedTargets
    return PackedTargets(targets, torch.device("cuda"))


# ---------------------------------------------------------------------------------------------------------- kernel tests
@pytest.mark.parametrize("case", ref.KERNEL_CASES, ids=str)
def test_cost_blocks_match_fp64(case):
    from myrtle_vision.hip import lib
    B, Q, C, sizes = case
    logits, boxes, targets, _, _ = ref.case_inputs(case)
    want = ref.case_reference(case, torch.float64)["cost"]
    p = pack(targets)
    g = Guarded()
    out = g.out((max(Q * p.total, 1),))
    lg, bx = logits.cuda(), boxes.cuda()
    rc = lib.lib().mv_det_cost(lg.data_ptr(), bx.data_ptr(), p.labels.data_ptr(), p.boxes.data_ptr(), p.toff.data_ptr(),
                               out.data_ptr(), 1.0, 1.0, 1.0, B, Q, C + 1, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    g.check()
    flat = out.cpu()
    worst = 0.0
    for b, n in enumerate(sizes):
        blk = flat[Q * p.offsets[b]:Q * (p.offsets[b] + n)].view(Q, n)
        assert blk.shape == want[b].shape and bool(torch.isfinite(blk).all())
        worst = max(worst, ref.relmax(blk, want[b]))
    assert bool(torch.isnan(flat[Q * p.total:]).all())                      # nothing beyond the packed blocks was written
    within("cost", worst, str(case))
    # other weights: the three terms are scaled separately
    from myrtle_vision.models.matcher import HungarianMatcher
    blocks = HungarianMatcher(cost_class=2.0, cost_bbox=0.5, cost_giou=3.0).cost_blocks({"pred_logits": lg, "pred_boxes": bx}, p)
    for b, t in enumerate(targets):
        if len(t["labels"]):
            w = ref.cost_block(logits[b].double(), boxes[b].double(), t["labels"], t["boxes"].double(), 2.0, 0.5, 3.0)
            assert ref.relmax(blocks[b], w) <= 4 * TABLE["cost"][1]                 # up to 3 x the weight on one term


@pytest.mark.parametrize("case", ref.KERNEL_CASES, ids=str)
def test_matcher_returns_the_reference_format_and_the_fp64_assignment(case):
    from myrtle_vision.models.matcher import HungarianMatcher
    B, Q, C, sizes = case
    logits, boxes, targets, _, _ = ref.case_inputs(case)
    want = ref.match(logits, boxes, targets)
    got = HungarianMatcher()({"pred_logits": logits.cuda(), "pred_boxes": boxes.cuda()},
                             [{k: v.cuda() for k, v in t.items()} for t in targets])
    assert len(got) == B
    for (i, j), (wi, wj), n in zip(got, want, sizes):
        assert i.dtype == j.dtype == torch.int64 and not i.is_cuda and not j.is_cuda
        assert len(i) == len(j) == min(Q, n)
        # same assignment unless the fp64 optimum has a near-tie: then the same total cost to fp32 accuracy
        if not (np.array_equal(i.numpy(), wi) and np.array_equal(j.numpy(), wj)):
            b = [x[0] is i for x in got].index(True)
            c = ref.cost_block(logits[b].double(), boxes[b].double(), targets[b]["labels"], targets[b]["boxes"].double())
            assert abs(float(c[i, j].sum() - c[wi, wj].sum())) < 1e-5


@pytest.mark.parametrize("case", ref.KERNEL_CASES, ids=str)
def test_loss_kernels_match_fp64(case):
    from myrtle_vision.hip import lib
    B, Q, C, sizes = case
    C1 = C + 1
    logits, boxes, targets, weight, _ = ref.case_inputs(case)
    want = ref.case_reference(case, torch.float64)
    p = pack(targets)
    match = np.full(B * Q, -1, dtype=np.int32)
    for b, (i, j) in enumerate(want["indices"]):
        match[b * Q + i] = p.offsets[b] + j
    match = torch.from_numpy(match).cuda()
    s = torch.cuda.current_stream().cuda_stream
    g = Guarded()
    tgt_class, tgt_box = g.out((B, Q), torch.int64), g.out((B, Q, 4))
    assert lib.lib().mv_det_assign(match.data_ptr(), p.labels.data_ptr(), p.boxes.data_ptr(), tgt_class.data_ptr(),
                                   tgt_box.data_ptr(), B * Q, p.total, C, s) == 0
    g.check()
    assert torch.equal(tgt_class.cpu(), want["tgt_class"]) and torch.equal(tgt_box.cpu(), want["tgt_box"].float())

    lg, bx, w = logits.cuda(), boxes.cuda(), weight.cuda()
    stats, lse = g.out((8,)), g.out((B * Q,))
    nb = want["num_boxes"]
    assert lib.lib().mv_det_loss_fwd(lg.data_ptr(), bx.data_ptr(), tgt_class.data_ptr(), tgt_box.data_ptr(), w.data_ptr(),
                                     p.tcount.data_ptr(), lse.data_ptr(), stats.data_ptr(), 1.0 / nb, B, Q, C1, s) == 0
    g.check()
    st = stats.cpu()
    for k, q in enumerate(("loss_ce", "loss_bbox", "loss_giou", "class_error", "cardinality_error")):
        within(q, ref.relmax(st[k], want[q]), str(case))
    assert float(st[6]) == sum(min(Q, n) for n in sizes) and float(st[7]) == 0.0
    assert ref.relmax(lse.cpu(), torch.logsumexp(logits.double(), -1).reshape(-1)) < 1e-6

    gin = [torch.tensor(v, device="cuda") for v in ref.GRADS_IN]
    dlogits, dboxes = g.out((B, Q, C1)), g.out((B, Q, 4))
    assert lib.lib().mv_det_loss_bwd(lg.data_ptr(), bx.data_ptr(), tgt_class.data_ptr(), tgt_box.data_ptr(), w.data_ptr(),
                                     lse.data_ptr(), stats.data_ptr(), gin[0].data_ptr(), gin[1].data_ptr(), gin[2].data_ptr(),
                                     dlogits.data_ptr(), dboxes.data_ptr(), 1.0 / nb, B, Q, C1, s) == 0
    g.check()
    within("dlogits", ref.relmax(dlogits, want["dlogits"]), str(case))
    within("dboxes", ref.relmax(dboxes, want["dboxes"]), str(case))
    unmatched = (want["tgt_class"] == C).cuda()
    assert bool((dboxes[unmatched] == 0).all())


@pytest.mark.parametrize("case", ref.KERNEL_CASES, ids=str)
def test_criterion_module_and_autograd_match_fp64(case):
    """SetCriterion end to end on the case (matcher included), gradients through the autograd function with the reference's loss
    weights; an unused loss (its incoming gradient is None) contributes nothing."""
    from myrtle_vision.models.detector import SetCriterion
    from myrtle_vision.models.matcher import HungarianMatcher
    B, Q, C, sizes = case
    logits, boxes, targets, _, _ = ref.case_inputs(case)
    want = ref.case_reference(case, torch.float64)
    crit = SetCriterion(C, HungarianMatcher(), {}, ref.EOS_COEF, ["labels", "boxes", "cardinality"]).cuda()
    lg, bx = logits.cuda().requires_grad_(True), boxes.cuda().requires_grad_(True)
    losses = crit({"pred_logits": lg, "pred_boxes": bx}, [{k: v.cuda() for k, v in t.items()} for t in targets])
    assert list(losses) == ["loss_ce", "class_error", "loss_bbox", "loss_giou", "cardinality_error"]
    assert not losses["class_error"].requires_grad and not losses["cardinality_error"].requires_grad
    for q in losses:
        within(q, ref.relmax(losses[q], want[q]), f"module {case}")
    (ref.GRADS_IN[0] * losses["loss_ce"] + ref.GRADS_IN[1] * losses["loss_bbox"] + ref.GRADS_IN[2] * losses["loss_giou"]).backward()
    within("dlogits", ref.relmax(lg.grad, want["dlogits"]), f"module {case}")
    within("dboxes", ref.relmax(bx.grad, want["dboxes"]), f"module {case}")
    only = SetCriterion(C, HungarianMatcher(), {}, ref.EOS_COEF, ["labels"]).cuda()
    lg2, bx2 = logits.cuda().requires_grad_(True), boxes.cuda().requires_grad_(True)
    out = only({"pred_logits": lg2, "pred_boxes": bx2}, targets)
    assert list(out) == ["loss_ce", "class_error"]
    out["loss_ce"].backward()
    assert bool((bx2.grad == 0).all()) if bx2.grad is not None else True


@pytest.mark.parametrize("case", ref.KERNEL_CASES, ids=str)
def test_postprocess_matches_fp64(case):
    from myrtle_vision.hip import lib
    from myrtle_vision.models.detector import PostProcess
    B, Q, C, sizes = case
    logits, boxes, _, _, img_sizes = ref.case_inputs(case)
    want = ref.case_reference(case, torch.float64)
    g = Guarded()
    scores, labels, out = g.out((B, Q)), g.out((B, Q), torch.int64), g.out((B, Q, 4))
    lg, bx, sz = logits.cuda(), boxes.cuda(), img_sizes.cuda()
    assert lib.lib().mv_det_postprocess(lg.data_ptr(), bx.data_ptr(), sz.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                        out.data_ptr(), B, Q, C + 1, torch.cuda.current_stream().cuda_stream) == 0
    g.check()
    within("pp_scores", ref.relmax(scores, want["pp_scores"]), str(case))
    within("pp_boxes", ref.relmax(out, want["pp_boxes"]), str(case))
    assert torch.equal(labels.cpu(), want["pp_labels"])
    res = PostProcess()({"pred_logits": lg, "pred_boxes": bx}, img_sizes.long().cuda())
    assert len(res) == B and list(res[0]) == ["scores", "labels", "boxes"]
    assert torch.equal(torch.stack([r["labels"] for r in res]).cpu(), want["pp_labels"])
    assert torch.equal(torch.stack([r["boxes"] for r in res]), out)


@pytest.mark.parametrize("case", ref.HEAD_CASES, ids=str)
def test_heads_and_append_kernels_match_fp64(case):
    from myrtle_vision.hip import lib
    B, T, Q, D, C = case
    C1 = C + 1
    t = {k: v.cuda() for k, v in ref.head_inputs(case).items()}
    want = ref.head_reference(case, torch.float64)
    s = torch.cuda.current_stream().cuda_stream
    L = lib.lib()
    g = Guarded()
    logits, boxes = g.out((B, Q, C1)), g.out((B, Q, 4))
    assert L.mv_det_heads_fwd(t["x"].data_ptr(), t["wc"].data_ptr(), t["bc"].data_ptr(), t["wb"].data_ptr(), t["bb"].data_ptr(),
                              logits.data_ptr(), boxes.data_ptr(), B, T, Q, D, C1, s) == 0
    g.check()
    within("head_logits", ref.relmax(logits, want["head_logits"]), str(case))
    within("head_boxes", ref.relmax(boxes, want["head_boxes"]), str(case))
    dx = g.out((B, T, D))
    dx.zero_()
    dwc, dbc, dwb, dbb = g.out((C1, D)), g.out((C1,)), g.out((4, D)), g.out((4,))
    nws = L.mv_det_heads_bwd_workspace_bytes(B, Q, D, C1)
    ws = g.out((nws // 4,))
    assert L.mv_det_heads_bwd(t["x"].data_ptr(), t["wc"].data_ptr(), t["wb"].data_ptr(), boxes.data_ptr(), t["dlogits"].data_ptr(),
                              t["dboxes"].data_ptr(), dx.data_ptr(), dwc.data_ptr(), dbc.data_ptr(), dwb.data_ptr(),
                              dbb.data_ptr(), ws.data_ptr(), nws, B, T, Q, D, C1, s) == 0
    g.check()
    for q, got in (("head_dx", dx), ("head_dw_cls", dwc), ("head_db_cls", dbc), ("head_dw_box", dwb), ("head_db_box", dbb)):
        within(q, ref.relmax(got, want[q]), str(case))
    assert bool((dx[:, :T - Q] == 0).all())                                   # rows the decoder does not read: untouched
    # the append pair
    seq = g.out((B, T + Q, D))
    det, pos = t["det"].view(Q, D), t["pos"].view(Q, D)
    assert L.mv_det_append_fwd(t["x"].data_ptr(), det.data_ptr(), pos.data_ptr(), seq.data_ptr(), B, T, Q, D, s) == 0
    adx, ddet, dpos = g.out((B, T, D)), g.out((Q, D)), g.out((Q, D))
    assert L.mv_det_append_bwd(t["dout"].data_ptr(), adx.data_ptr(), ddet.data_ptr(), dpos.data_ptr(), B, T, Q, D, s) == 0
    g.check()
    for q, got in (("append_out", seq), ("append_dx", adx), ("append_ddet", ddet), ("append_dpos", dpos)):
        within(q, ref.relmax(got, want[q]), str(case))
    assert torch.equal(ddet, dpos)


def test_entry_points_reject_bad_shapes_and_write_nothing():
    from myrtle_vision.hip import lib
    L = lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = Guarded()
    out = g.out((64,))
    z = torch.zeros(64, device="cuda")
    zi = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert L.mv_det_cost(z.data_ptr(), z.data_ptr(), zi.data_ptr(), z.data_ptr(), zi.data_ptr(), out.data_ptr(), 1.0, 1.0, 1.0, 0,
                         4, 3, s) == -1
    assert L.mv_det_heads_fwd(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), out.data_ptr(), out.data_ptr(),
                              1, 2, 4, 8, 3, s) == -1                       # more queries than tokens
    assert L.mv_det_loss_fwd(z.data_ptr(), z.data_ptr(), zi.data_ptr(), z.data_ptr(), z.data_ptr(), zi.data_ptr(), out.data_ptr(),
                             out.data_ptr(), 1.0, 1, 4, 1, s) == -1         # no class besides "no object"
    g.check()
    assert bool(torch.isnan(out).all())


def test_out_of_range_label_poisons_instead_of_indexing():
    from myrtle_vision.models.detector import SetCriterion
    B, Q, C = 1, 4, 3
    lg, bx = torch.randn(B, Q, C + 1).cuda(), torch.full((B, Q, 4), 0.5).cuda()

    class Fixed:
        def __call__(self, outputs, targets):
            return [(torch.tensor([0]), torch.tensor([0]))]
    crit = SetCriterion(C, Fixed(), {}, 0.1, ["labels"]).cuda()
    out = crit({"pred_logits": lg, "pred_boxes": bx}, [{"labels": torch.tensor([7]).cuda(), "boxes": torch.full((1, 4), 0.5).cuda()}])
    assert bool(torch.isnan(out["loss_ce"]))


# ---------------------------------------------------------------------------------------------------------- model goldens
def build(name, precision, **extra):
    from myrtle_vision.models.vit import ViT
    arrays, meta = load_golden(name)
    vit = ViT(patch_size=16, q_format="FP32", precision=precision, **meta["kwargs"], **extra)
    sd = vit.state_dict()
    assert list(sd.keys()) == meta["state_keys"]
    vit.load_state_dict({k: det_param(k, v.shape) for k, v in sd.items()})
    vit = vit.cuda().train()
    img = det_images(name, meta["batch"], meta["kwargs"]["image_size"]).cuda()
    targets = [{"labels": torch.from_numpy(arrays[f"tgt_labels:{b}"]).cuda(), "boxes": torch.from_numpy(arrays[f"tgt_boxes:{b}"]).cuda()}
               for b in range(meta["batch"])]
    return vit, img, targets, arrays, meta


class FixedMatcher:
    """Hands the fixture's indices to the criterion (bf16: only the loss arithmetic is judged)."""

    def __init__(self, arrays, batch):
        self.indices = [(torch.from_numpy(arrays[f"index_i:{b}"]), torch.from_numpy(arrays[f"index_j:{b}"])) for b in range(batch)]

    def __call__(self, outputs, targets):
        return self.indices


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["micro_det", "base_det"])
def test_detection_model_matches_reference(name, precision):
    """Outputs, matcher indices, the five criterion values, the weighted total and every gradient summary against the reference's
    fixture, at the project's per-precision bars.
    The fixtures' matched boxes keep clear of the points where L1's sign or a GIoU max / min / clamp selection changes (the
    generator's kink check, tests/golden/gen_golden_detection.py): on such a point the gradient jumps, and a comparison at any
    tolerance would judge the direction of a rounding.  (An earlier micro_det with coordinates 7e-4 from their targets did exactly
    that in bf16: every gradient 14-22 % away in relative L2 with norms equal to 3 %.)"""
    from myrtle_vision.models.detector import SetCriterion
    from myrtle_vision.models.matcher import HungarianMatcher
    vit, img, targets, arrays, meta = build(name, precision)
    tol, tol_grad = TOL_OUT[precision], TOL_GRAD[precision]
    out = vit(img)
    assert set(out) == {"pred_logits", "pred_boxes"}
    assert out["pred_logits"].dtype == out["pred_boxes"].dtype == torch.float32
    for k in ("pred_logits", "pred_boxes"):
        e = ref.relmax(out[k], arrays[k])
        report(f"{name}/{precision} {k}", e)
        assert e < tol, (k, e)
    if precision in EXACT:
        assert np.array_equal(out["pred_logits"].argmax(-1).cpu().numpy(), arrays["pred_logits"].argmax(-1))
        matcher = HungarianMatcher()
        for b, (i, j) in enumerate(matcher(out, targets)):
            assert np.array_equal(i.numpy(), arrays[f"index_i:{b}"]) and np.array_equal(j.numpy(), arrays[f"index_j:{b}"]), b
    else:
        matcher = FixedMatcher(arrays, meta["batch"])
    wd = meta["weight_dict"]
    crit = SetCriterion(meta["kwargs"]["num_classes"], matcher, wd, meta["eos_coef"], meta["losses"]).cuda()
    losses = crit(out, targets)
    assert set(losses) == {"loss_ce", "class_error", "cardinality_error", "loss_bbox", "loss_giou"}
    total = sum(losses[k] * wd[k] for k in losses if k in wd)
    keys = list(losses) if precision in EXACT else ["loss_ce", "loss_bbox", "loss_giou"]
    for k in keys:
        e = abs(float(losses[k].detach()) - float(arrays[k])) / max(1.0, abs(float(arrays[k])))
        report(f"{name}/{precision} {k}", e)
        assert e < tol, (k, float(losses[k].detach()), float(arrays[k]))
    assert abs(float(total.detach()) - float(arrays["total"])) < tol * max(1.0, abs(float(arrays["total"])))
    total.backward()
    torch.cuda.synchronize()
    unused, worst = [], 0.0
    for pname, p in vit.named_parameters():
        if p.grad is None:
            unused.append(pname)
            continue
        w = arrays[f"gsum:{pname}"]
        got = summarize(p.grad.float().cpu()).numpy()
        if precision in EXACT:
            e = max(np.abs(got[:4] - w[:4]).max() / max(w[1], 1e-30), np.abs(got[4:] - w[4:]).max() / max(w[2], 1e-30))
        else:
            e = max(abs(got[1] - w[1]) / max(w[1], 1e-30), abs(got[2] - w[2]) / max(w[2], 1e-30),
                    np.abs(got[4:] - w[4:]).max() / max(w[2], 1e-30))
        worst = max(worst, e)
        assert e < tol_grad, (pname, e)
        if f"grad:{pname}" in arrays:
            assert ref.relmax(p.grad, arrays[f"grad:{pname}"]) < tol_grad, pname
    report(f"{name}/{precision} grad-summaries", worst)
    assert sorted(unused) == sorted(meta["unused_params"]) == sorted(vit.unused_parameter_names())


def test_hooked_head_falls_back_to_module_by_module():
    vit, img, _, arrays, _ = build("micro_det", "fp32")
    seen = []
    h = vit.decoder.bbox_embed.register_forward_hook(lambda m, a, o: seen.append(tuple(o.shape)))
    out = vit(img)
    h.remove()
    assert seen == [(3, 100, 4)]
    assert ref.relmax(out["pred_logits"], arrays["pred_logits"]) < 1e-3 and ref.relmax(out["pred_boxes"], arrays["pred_boxes"]) < 1e-3


# ------------------------------------------------------------------------------------------------------- live det tokens
def _live_reference(params, img, targets, indices, cfg, eos):
    """CPU fp32 torch restatement of the branch YOLOS intends (reference vit.py:285-302 with ``decoder == "detection"`` true):
    cat(cls, patches, det_tokens) + cat(pos_cls, resized grid, pos_embedding_det), the transformer, the heads, the set loss."""
    import torch.nn.functional as TF
    from oracle.vit_oracle import gelu_erf, layer_norm, patchify, resized_pos_embedding
    P = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    b, _, h, w = img.shape
    p, H, Q, C = 16, cfg["heads"], 100, cfg["num_classes"]
    x = TF.linear(patchify(img, p), P["patch_to_embedding.weight"], P["patch_to_embedding.bias"])
    x = torch.cat((P["cls_token"].expand(b, -1, -1), x, P["det_tokens"].expand(b, -1, -1)), dim=1)
    x = x + torch.cat((resized_pos_embedding(P["pos_embedding"], h // p, w // p), P["pos_embedding_det"]), dim=1)
    for i in range(cfg["depth"]):
        pre = f"transformer.layers.{i}"
        y = layer_norm(x, P[f"{pre}.0.fn.norm.weight"], P[f"{pre}.0.fn.norm.bias"])
        n, c = y.shape[1], y.shape[2]
        qkv = TF.linear(y, P[f"{pre}.0.fn.fn.to_qkv.weight"], P[f"{pre}.0.fn.fn.to_qkv.bias"])
        qkv = qkv.reshape(b, n, 3, H, c // H).permute(2, 0, 3, 1, 4)
        attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * 64 ** -0.5).softmax(dim=-1)
        o = (attn @ qkv[2]).transpose(1, 2).reshape(b, n, c)
        x = TF.linear(o, P[f"{pre}.0.fn.fn.to_out.0.weight"], P[f"{pre}.0.fn.fn.to_out.0.bias"]) + x
        y = layer_norm(x, P[f"{pre}.1.fn.norm.weight"], P[f"{pre}.1.fn.norm.bias"])
        hdn = gelu_erf(TF.linear(y, P[f"{pre}.1.fn.fn.net.0.weight"], P[f"{pre}.1.fn.fn.net.0.bias"]))
        x = TF.linear(hdn, P[f"{pre}.1.fn.fn.net.3.weight"], P[f"{pre}.1.fn.fn.net.3.bias"]) + x
    logits, boxes = ref.heads(x, P["decoder.class_embed.weight"], P["decoder.class_embed.bias"], P["decoder.bbox_embed.weight"],
                              P["decoder.bbox_embed.bias"], Q)
    tc, tb = ref.per_query_targets(indices, targets, b, Q, C, torch.float32)
    weight = torch.ones(C + 1)
    weight[-1] = eos
    sizes = [len(t["labels"]) for t in targets]
    ce, l1, gi, _, _ = ref.set_losses(logits, boxes, tc, tb, weight, torch.tensor(sizes), max(float(sum(sizes)), 1.0))
    total = ce + 5.0 * l1 + 2.0 * gi
    total.backward()
    return logits.detach(), boxes.detach(), total.detach(), {k: v.grad for k, v in P.items()}


def _live_step(vit, img, targets, matcher, meta):
    from myrtle_vision.models.detector import SetCriterion
    crit = SetCriterion(meta["kwargs"]["num_classes"], matcher, {}, meta["eos_coef"], ["labels", "boxes"]).cuda()
    out = vit(img)
    losses = crit(out, targets)
    total = losses["loss_ce"] + 5.0 * losses["loss_bbox"] + 2.0 * losses["loss_giou"]
    return out, total


def test_live_det_tokens_match_the_intended_branch_and_train():
    """Opt-in sequence assembly (297 tokens): outputs and ALL gradients, det_tokens and pos_embedding_det included, against the CPU
    fp32 restatement; nothing is unused; two backward passes give bit-identical gradients; one AdamW step through ParamArena moves
    both parameters."""
    from myrtle_vision.models.matcher import HungarianMatcher
    from myrtle_vision.utils.optim import AdamW, ParamArena
    vit, img, targets, arrays, meta = build("micro_det", "fp32", live_det_tokens=True)
    assert vit.unused_parameter_names() == ()
    out, total = _live_step(vit, img, targets, HungarianMatcher(), meta)
    assert out["pred_logits"].shape == (3, 100, 21)
    indices = HungarianMatcher()(out, targets)
    total.backward()
    grads = {n: p.grad.detach().clone() for n, p in vit.named_parameters()}
    assert all(p.grad is not None for p in vit.parameters())

    cpu_targets = [{k: v.cpu() for k, v in t.items()} for t in targets]
    params = {k: v.detach().cpu() for k, v in vit.state_dict().items()}
    rl, rb, rt, rg = _live_reference(params, img.cpu(), cpu_targets, [(i.numpy(), j.numpy()) for i, j in indices], meta["kwargs"],
                                     meta["eos_coef"])
    assert ref.relmax(out["pred_logits"], rl) < 1e-3 and ref.relmax(out["pred_boxes"], rb) < 1e-3
    assert np.array_equal(out["pred_logits"].argmax(-1).cpu().numpy(), rl.argmax(-1).numpy())
    assert abs(float(total) - float(rt)) < 1e-3 * max(1.0, abs(float(rt)))
    for n, gr in grads.items():
        e = float((gr.cpu() - rg[n]).norm() / rg[n].norm().clamp_min(1e-30))
        report(f"live-det-tokens grad {n}", e)
        assert e < 1e-3, (n, e)
    assert float(grads["det_tokens"].abs().max()) > 0 and float(grads["pos_embedding_det"].abs().max()) > 0
    assert torch.equal(grads["det_tokens"], grads["pos_embedding_det"])

    # determinism: the same step again, bit for bit
    for p in vit.parameters():
        p.grad = None
    _, total2 = _live_step(vit, img, targets, HungarianMatcher(), meta)
    total2.backward()
    assert torch.equal(total2, total)
    for n, p in vit.named_parameters():
        assert torch.equal(p.grad, grads[n]), n

    # one optimizer step through the arena
    vit2, img, targets, _, meta = build("micro_det", "fp32", live_det_tokens=True)
    opt = AdamW(ParamArena(vit2.named_parameters(), skip=vit2.unused_parameter_names()), lr=1e-3, weight_decay=0.05)
    before = {n: p.detach().clone() for n, p in vit2.named_parameters()}
    opt.zero_grad()
    _, t3 = _live_step(vit2, img, targets, HungarianMatcher(), meta)
    t3.backward()
    opt.step()
    torch.cuda.synchronize()
    for n in ("det_tokens", "pos_embedding_det", "decoder.class_embed.weight", "decoder.bbox_embed.bias"):
        p = dict(vit2.named_parameters())[n]
        assert bool(torch.isfinite(p).all()) and float((p.detach() - before[n]).abs().max()) > 0, n


@pytest.mark.parametrize("precision", ["bf16", "bf16x3h"])
def test_live_det_tokens_run_in_the_other_precisions(precision):
    """297 tokens: bf16 stays on the whole-head attention kernels, bf16x3h crosses to the key-tiled ones; both against fp32."""
    from myrtle_vision.models.matcher import HungarianMatcher
    vit, img, targets, _, meta = build("micro_det", "fp32", live_det_tokens=True)
    with torch.no_grad():
        want = vit(img)
    other, _, _, _, _ = build("micro_det", precision, live_det_tokens=True)
    out, total = _live_step(other, img, targets, HungarianMatcher(), meta)
    tol = 1.5e-2 if precision == "bf16" else 1e-3
    assert ref.relmax(out["pred_logits"], want["pred_logits"]) < tol and ref.relmax(out["pred_boxes"], want["pred_boxes"]) < tol
    total.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in other.parameters())


def test_no_targets_in_the_batch_clamps_num_boxes_and_stays_finite():
    from myrtle_vision.models.detector import SetCriterion
    from myrtle_vision.models.matcher import HungarianMatcher
    vit, img, _, _, meta = build("micro_det", "fp32")
    empty = [{"labels": torch.zeros(0, dtype=torch.int64).cuda(), "boxes": torch.zeros(0, 4).cuda()} for _ in range(meta["batch"])]
    crit = SetCriterion(meta["kwargs"]["num_classes"], HungarianMatcher(), {}, meta["eos_coef"], meta["losses"]).cuda()
    assert crit.num_boxes(empty, img.device) == 1.0
    out = vit(img)
    assert all(len(i) == 0 and len(j) == 0 and i.dtype == torch.int64 for i, j in HungarianMatcher()(out, empty))
    losses = crit(out, empty)
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert float(losses["loss_bbox"]) == 0.0 and float(losses["loss_giou"]) == 0.0 and float(losses["class_error"]) == 100.0
    (losses["loss_ce"] + 5 * losses["loss_bbox"] + 2 * losses["loss_giou"]).backward()
    assert all(bool(torch.isfinite(p.grad).all()) for n, p in vit.named_parameters() if p.grad is not None)
    assert float(vit.decoder.bbox_embed.weight.grad.abs().max()) == 0.0
