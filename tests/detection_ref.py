"""Restatement of the YOLOS tail in plain torch, dtype-generic (fp32 or fp64): the checker of tests/test_detection_gpu.py, the
fp32-against-fp64 baseline of profiles/detection_parity.txt and the torch side of tools/bench_detection_tail.py.  Formulas:
torchvision.ops.boxes (box_convert, generalized_box_iou: no epsilon), reference models/matcher.py:58-82, models/detector.py:41-98,
159-176.  Not a test module (no test_ prefix): imported by them."""
import numpy as np
import torch
import torch.nn.functional as TF
from scipy.optimize import linear_sum_assignment


def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)


def giou(a, b):
    """Generalized IoU of xyxy boxes, broadcasting over the leading dimensions."""
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a + area_b - inter
    whi = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    areai = whi[..., 0] * whi[..., 1]
    return inter / union - (areai - union) / areai


def cost_block(logits, boxes, labels, tboxes, cost_class=1.0, cost_bbox=1.0, cost_giou=1.0):
    """One image: logits [Q, C1], boxes [Q, 4], labels [T], tboxes [T, 4] -> [Q, T]."""
    prob = logits.softmax(-1)
    l1 = (boxes[:, None, :] - tboxes[None, :, :]).abs().sum(-1)
    g = giou(xyxy(boxes)[:, None, :], xyxy(tboxes)[None, :, :])
    return cost_bbox * l1 - cost_class * prob[:, labels] - cost_giou * g


def match(logits, boxes, targets):
    """scipy on the fp64 cost blocks -> [(index_i, index_j)] (numpy int64)."""
    out = []
    for b, t in enumerate(targets):
        if len(t["labels"]) == 0:
            out.append((np.zeros(0, np.int64), np.zeros(0, np.int64)))
            continue
        c = cost_block(logits[b].double(), boxes[b].double(), t["labels"], t["boxes"].double())
        i, j = linear_sum_assignment(c.numpy())
        out.append((i.astype(np.int64), j.astype(np.int64)))
    return out


def per_query_targets(indices, targets, B, Q, num_classes, dtype):
    tgt_class = torch.full((B, Q), num_classes, dtype=torch.int64)
    tgt_box = torch.zeros(B, Q, 4, dtype=dtype)
    for b, (i, j) in enumerate(indices):
        if len(i):
            tgt_class[b, torch.as_tensor(i)] = targets[b]["labels"][torch.as_tensor(j)]
            tgt_box[b, torch.as_tensor(i)] = targets[b]["boxes"][torch.as_tensor(j)].to(dtype)
    return tgt_class, tgt_box


def set_losses(logits, boxes, tgt_class, tgt_box, weight, tcount, num_boxes):
    """-> (loss_ce, loss_bbox, loss_giou, class_error, cardinality_error) in the dtype of ``logits``."""
    C1 = logits.shape[-1]
    ce = TF.cross_entropy(logits.reshape(-1, C1), tgt_class.reshape(-1), weight.to(logits.dtype))
    m = tgt_class != C1 - 1
    l1 = (boxes[m] - tgt_box[m]).abs().sum() / num_boxes
    gi = (1 - giou(xyxy(boxes[m]), xyxy(tgt_box[m]))).sum() / num_boxes
    am = logits.argmax(-1)
    if bool(m.any()):
        class_error = 100 - (am[m] == tgt_class[m]).to(logits.dtype).sum() * (100.0 / int(m.sum()))
    else:
        class_error = torch.tensor(100.0, dtype=logits.dtype)
    card = ((am != C1 - 1).sum(1).to(logits.dtype) - tcount.to(logits.dtype)).abs().mean()
    return ce, l1, gi, class_error, card


def postprocess(logits, boxes, sizes):
    prob = logits.softmax(-1)
    scores, labels = prob[..., :-1].max(-1)
    h, w = sizes.to(logits.dtype).unbind(1)
    return scores, labels, xyxy(boxes) * torch.stack([w, h, w, h], dim=1)[:, None, :]


def heads(x, wc, bc, wb, bb, Q):
    x = x[:, -Q:, :]
    return TF.linear(x, wc, bc), TF.linear(x, wb, bb).sigmoid()


def append(x, det, pos):
    return torch.cat((x, (det + pos).expand(x.shape[0], -1, -1)), dim=1)


# ---- deterministic inputs of the kernel cases -------------------------------------------------------------------------------
# (B, Q, C, target counts): ragged counts with zeros, Q in {1, 100, 128}, C in {1, 20, 91}, images whose targets outnumber the
# queries (Q = 1 with 3 targets, Q = 4 with 9), a batch with no target at all
KERNEL_CASES = [(3, 100, 20, (0, 6, 12)), (2, 1, 1, (3, 0)), (4, 128, 91, (30, 1, 0, 7)), (2, 100, 1, (5, 2)), (1, 128, 20, (0,)),
                (2, 4, 20, (9, 2)), (2, 100, 91, (12, 30))]
GRADS_IN = (1.0, 5.0, 2.0)        # incoming gradients of (loss_ce, loss_bbox, loss_giou): the reference's weight_dict
EOS_COEF = 0.1


def _boxes(g, *shape):
    u = torch.rand(*shape, 4, generator=g, dtype=torch.float64)
    return torch.stack((0.2 + 0.6 * u[..., 0], 0.2 + 0.6 * u[..., 1], 0.05 + 0.45 * u[..., 2], 0.05 + 0.45 * u[..., 3]), dim=-1).float()


def case_inputs(case):
    """fp32 CPU inputs of one kernel case (a function of the case alone)."""
    B, Q, C, sizes = case
    g = torch.Generator().manual_seed(1000 * B + 10 * Q + C)
    logits = (2.0 * torch.randn(B, Q, C + 1, generator=g, dtype=torch.float64)).float()
    boxes = _boxes(g, B, Q)
    targets = [{"labels": torch.randint(0, C, (n,), generator=g), "boxes": _boxes(g, n)} for n in sizes]
    weight = torch.ones(C + 1)
    weight[-1] = EOS_COEF
    img_sizes = torch.randint(200, 1000, (B, 2), generator=g).float()
    return logits, boxes, targets, weight, img_sizes


def case_reference(case, dtype):
    """Every quantity of one case evaluated by torch on the CPU in ``dtype`` (matching: always the fp64 one)."""
    B, Q, C, sizes = case
    logits, boxes, targets, weight, img_sizes = case_inputs(case)
    indices = match(logits, boxes, targets)
    out = {"indices": indices}
    out["cost"] = [cost_block(logits[b].to(dtype), boxes[b].to(dtype), t["labels"], t["boxes"].to(dtype))
                   for b, t in enumerate(targets)]
    tgt_class, tgt_box = per_query_targets(indices, targets, B, Q, C, dtype)
    lg, bx = logits.to(dtype).requires_grad_(True), boxes.to(dtype).requires_grad_(True)
    num_boxes = max(float(sum(sizes)), 1.0)
    ce, l1, gi, cerr, card = set_losses(lg, bx, tgt_class, tgt_box, weight, torch.tensor(sizes), num_boxes)
    (GRADS_IN[0] * ce + GRADS_IN[1] * l1 + GRADS_IN[2] * gi).backward()
    out.update(loss_ce=ce.detach(), loss_bbox=l1.detach(), loss_giou=gi.detach(), class_error=cerr.detach(),
               cardinality_error=card.detach(), dlogits=lg.grad, dboxes=bx.grad if bx.grad is not None else torch.zeros_like(bx),
               tgt_class=tgt_class, tgt_box=tgt_box, num_boxes=num_boxes)
    s, l, b = postprocess(logits.to(dtype), boxes.to(dtype), img_sizes)
    out.update(pp_scores=s, pp_labels=l, pp_boxes=b)
    return out


HEAD_CASES = [(2, 197, 100, 192, 20), (3, 297, 100, 768, 20), (1, 130, 128, 64, 91), (5, 17, 1, 192, 1)]   # (B, T, Q, D, C)


def head_inputs(case):
    B, T, Q, D, C = case
    g = torch.Generator().manual_seed(7 * B + T + Q + D + C)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()          # noqa: E731
    return dict(x=r(B, T, D), wc=r(C + 1, D) * D ** -0.5, bc=0.1 * r(C + 1), wb=r(4, D) * D ** -0.5, bb=0.1 * r(4),
                dlogits=r(B, Q, C + 1), dboxes=r(B, Q, 4), det=0.5 * r(1, Q, D), pos=0.5 * r(1, Q, D), dout=r(B, T + Q, D))


def head_reference(case, dtype):
    B, T, Q, D, C = case
    t = {k: v.to(dtype) for k, v in head_inputs(case).items()}
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("x", "wc", "bc", "wb", "bb")}
    logits, boxes = heads(leaves["x"], leaves["wc"], leaves["bc"], leaves["wb"], leaves["bb"], Q)
    ((logits * t["dlogits"]).sum() + (boxes * t["dboxes"]).sum()).backward()
    out = dict(head_logits=logits.detach(), head_boxes=boxes.detach(), head_dx=leaves["x"].grad, head_dw_cls=leaves["wc"].grad,
               head_db_cls=leaves["bc"].grad, head_dw_box=leaves["wb"].grad, head_db_box=leaves["bb"].grad)
    al = {k: t[k].clone().requires_grad_(True) for k in ("x", "det", "pos")}
    seq = append(al["x"], al["det"], al["pos"])
    (seq * t["dout"]).sum().backward()
    out.update(append_out=seq.detach(), append_dx=al["x"].grad, append_ddet=al["det"].grad[0], append_dpos=al["pos"].grad[0])
    return out


def relmax(got, want):
    """max |got - want| / max |want| (1 when ``want`` is all zero), in fp64."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    if want.numel() == 0:
        return 0.0
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / (scale if scale > 0 else 1.0)


QUANTITIES = ("cost", "loss_ce", "loss_bbox", "loss_giou", "class_error", "cardinality_error", "dlogits", "dboxes", "pp_scores",
              "pp_boxes", "head_logits", "head_boxes", "head_dx", "head_dw_cls", "head_db_cls", "head_dw_box", "head_db_box",
              "append_out", "append_dx", "append_ddet", "append_dpos")


def fp32_baseline():
    """{quantity: the largest relmax of torch's fp32 CPU evaluation against its fp64 one over the cases}."""
    worst = {q: 0.0 for q in QUANTITIES}
    for case in KERNEL_CASES:
        a, b = case_reference(case, torch.float32), case_reference(case, torch.float64)
        for q in QUANTITIES[:10]:
            if q == "cost":
                e = max([relmax(x, y) for x, y in zip(a[q], b[q])] or [0.0])
            else:
                e = relmax(a[q], b[q])
            worst[q] = max(worst[q], e)
    for case in HEAD_CASES:
        a, b = head_reference(case, torch.float32), head_reference(case, torch.float64)
        for q in QUANTITIES[10:]:
            worst[q] = max(worst[q], relmax(a[q], b[q]))
    return worst


PARITY_FACTOR = 8.0


def write_parity_table(path):
    base = fp32_baseline()
    with open(path, "w") as f:
        f.write("# Detection tail kernels: tolerance table of tests/test_detection_gpu.py.\n"
                "# baseline = max over the cases of max|fp32 - fp64| / max|fp64| for torch's own fp32 evaluation of the same formulas\n"
                "# on the CPU (tests/detection_ref.py); bound = 8 x baseline (the kernels sum in another order and are still fp32).\n"
                "# Regenerate: python tests/detection_ref.py\n"
                "# quantity baseline bound\n")
        for q in QUANTITIES:
            f.write(f"{q} {base[q]:.6e} {PARITY_FACTOR * base[q]:.6e}\n")


def read_parity_table(path):
    table = {}
    with open(path) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            q, base, bound = line.split()[:3]
            table[q] = (float(base), float(bound))
    return table


if __name__ == "__main__":
    import os
    write_parity_table(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "detection_parity.txt"))
