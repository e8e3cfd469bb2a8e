#!/usr/bin/env python3
"""The YOLOS detection tail -- decoder + Hungarian matcher + set criterion, forward and backward -- on the HIP kernels of
csrc/detection.hip against a torch composition of the same formulas on the same device, in one process.

ViT-B width (D = 768), N = 197 tokens, Q = 100 queries, C = 20 classes, B in {2, 64}, 1..30 targets per image.  Both arms start
from the same transformer output x [B, N, D] (requires_grad) and the same targets on the device, and end with x.grad and the four
head gradients; both solve the assignment with scipy on the host.  The torch arm is the reference's arithmetic (matcher.py:58-86,
detector.py:41-138) with tests/detection_ref.py's box functions in place of torchvision's.  Per case, alternating in one process,
ROUNDS rounds; reported: the best round of each arm and its spread (slowest / fastest - 1), wall clock per step including the host
work (the matcher synchronises, so a step is one synchronised unit in both arms).

    python tools/bench_detection_tail.py [--out FILE]

--assignment host|device|both chooses where the HIP arm solves the assignment (HungarianMatcher's ``assignment``).  ``both``
times the HIP tail with the host matcher (scipy after a copy of the cost blocks) against the same tail with the device matcher
(mv_det_match), alternating inside every round, instead of HIP against torch: B in {2, 64} with 1..30 targets per image and
B = 2 with 100 targets per image (the solver's longest serial chain), MATCH_ROUNDS rounds of MATCH_ITERS steps.  The ``host``
and ``device`` arms pack the targets inside every step, as a training step does (its targets are new every time); that packing
is host work and a pageable host-to-device copy of the offsets.  The third arm, ``device_packed``, packs them once beforehand
(``SetCriterion.forward(..., packed=)``): the tail with no host dependency at all.

--profile-case I (with --assignment both) runs PROFILE_STEPS ``device_packed`` steps of case I and nothing else: the run to put
under ``rocprofv3 --kernel-trace --stats`` for det_match_kernel's own time."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "myrtle-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

import detection_ref as ref  # noqa: E402
from myrtle_vision.models.detector import SetCriterion  # noqa: E402
from myrtle_vision.models.matcher import HungarianMatcher, PackedTargets  # noqa: E402
from myrtle_vision.models.vit import DetectionDecoder  # noqa: E402

ROUNDS, ITERS = 3, 20
MATCH_ROUNDS, MATCH_ITERS = 5, 500
PROFILE_STEPS = 100
MATCH_CASES = ((2, None), (64, None), (2, 100))       # (B, targets per image; None = 1..30)
D, N, Q, C = 768, 197, 100, 20
WEIGHTS = {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0}
EOS = 0.1


def make_case(B, gen, fixed_targets=None):
    x = torch.randn(B, N, D, generator=gen).cuda().requires_grad_(True)
    dec = DetectionDecoder(D, C, Q).cuda()
    targets = []
    for _ in range(B):
        n = int(torch.randint(1, 31, (1,), generator=gen)) if fixed_targets is None else fixed_targets
        u = torch.rand(n, 4, generator=gen)
        boxes = torch.stack((0.2 + 0.6 * u[:, 0], 0.2 + 0.6 * u[:, 1], 0.05 + 0.45 * u[:, 2], 0.05 + 0.45 * u[:, 3]), -1)
        targets.append({"labels": torch.randint(0, C, (n,), generator=gen).cuda(), "boxes": boxes.cuda()})
    return x, dec, targets


def hip_arm(x, dec, targets, assignment="host", packed=None):
    crit = SetCriterion(C, HungarianMatcher(assignment=assignment), WEIGHTS, EOS, ["labels", "boxes", "cardinality"]).cuda()
    params = list(dec.parameters())

    def step():
        x.grad = None
        for p in params:
            p.grad = None
        losses = crit(dec(x), targets, packed=packed)
        sum(losses[k] * w for k, w in WEIGHTS.items()).backward()
        return losses
    return step


def torch_arm(x, dec, targets):
    wc, bc, wb, bb = dec.class_embed.weight, dec.class_embed.bias, dec.bbox_embed.weight, dec.bbox_embed.bias
    weight = torch.ones(C + 1, device="cuda")
    weight[-1] = EOS
    params = [wc, bc, wb, bb]

    def step():
        x.grad = None
        for p in params:
            p.grad = None
        logits, boxes = ref.heads(x, wc, bc, wb, bb, Q)
        B = logits.shape[0]
        with torch.no_grad():                                           # matcher.py:58-86
            prob = logits.flatten(0, 1).softmax(-1)
            ob = boxes.flatten(0, 1)
            ids = torch.cat([t["labels"] for t in targets])
            tb = torch.cat([t["boxes"] for t in targets])
            cost = torch.cdist(ob, tb, p=1) - prob[:, ids] - ref.giou(ref.xyxy(ob)[:, None, :], ref.xyxy(tb)[None, :, :])
            cost = cost.view(B, Q, -1).cpu()
            sizes = [len(t["boxes"]) for t in targets]
            indices = [linear_sum_assignment(c[i]) for i, c in enumerate(cost.split(sizes, -1))]
            indices = [(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in indices]
        num_boxes = max(float(sum(sizes)), 1.0)                          # detector.py:134-138, one process
        bidx = torch.cat([torch.full_like(s, i) for i, (s, _) in enumerate(indices)])
        sidx = torch.cat([s for s, _ in indices])
        tco = torch.cat([t["labels"][j] for t, (_, j) in zip(targets, indices)])
        tc = torch.full(logits.shape[:2], C, dtype=torch.int64, device="cuda")
        tc[bidx, sidx] = tco
        loss_ce = TF.cross_entropy(logits.transpose(1, 2), tc, weight)
        src = boxes[bidx, sidx]
        tgt = torch.cat([t["boxes"][j] for t, (_, j) in zip(targets, indices)], dim=0)
        loss_bbox = TF.l1_loss(src, tgt, reduction="none").sum() / num_boxes
        loss_giou = (1 - ref.giou(ref.xyxy(src), ref.xyxy(tgt))).sum() / num_boxes
        with torch.no_grad():
            class_error = 100 - (logits[bidx, sidx].argmax(-1) == tco).float().mean() * 100
            lengths = torch.as_tensor(sizes, device="cuda")
            card = TF.l1_loss((logits.argmax(-1) != C).sum(1).float(), lengths.float())
        (WEIGHTS["loss_ce"] * loss_ce + WEIGHTS["loss_bbox"] * loss_bbox + WEIGHTS["loss_giou"] * loss_giou).backward()
        return {"loss_ce": loss_ce, "loss_bbox": loss_bbox, "loss_giou": loss_giou, "class_error": class_error,
                "cardinality_error": card}
    return step


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6          # us, wall clock


def compare_assignments(args, dev):
    """HIP tail, host matcher against device matcher."""
    gen = torch.Generator().manual_seed(0)
    rows, lines = [], []
    for case, (B, fixed) in enumerate(MATCH_CASES):
        x, dec, targets = make_case(B, gen, fixed)
        arms = {k: hip_arm(x, dec, targets, k) for k in ("host", "device")}
        arms["device_packed"] = hip_arm(x, dec, targets, "device", PackedTargets(targets, x.device))
        if args.profile_case is not None:
            if case == args.profile_case:
                timeit(arms["device_packed"], PROFILE_STEPS)
            continue
        a = arms["host"]()
        gx = x.grad.clone()
        b = arms["device"]()
        same = all(torch.equal(a[k].detach(), b[k].detach()) for k in a) and torch.equal(gx, x.grad)
        b = arms["device_packed"]()
        same = same and all(torch.equal(a[k].detach(), b[k].detach()) for k in a) and torch.equal(gx, x.grad)
        times = {k: [] for k in arms}
        for _ in range(MATCH_ROUNDS):
            for k, fn in arms.items():                       # arms alternate inside a round
                times[k].append(timeit(fn, MATCH_ITERS))
        best = {k: min(v) for k, v in times.items()}
        spread = {k: max(v) / min(v) - 1 for k, v in times.items()}
        rec = {"B": B, "N": N, "D": D, "Q": Q, "C": C, "targets": sum(len(t["labels"]) for t in targets),
               "max_targets": max(len(t["labels"]) for t in targets), "device": dev, "rounds": MATCH_ROUNDS, "iters": MATCH_ITERS,
               "host_us": round(best["host"], 1), "device_us": round(best["device"], 1),
               "device_packed_us": round(best["device_packed"], 1),
               "host_spread": round(spread["host"], 4), "device_spread": round(spread["device"], 4),
               "device_packed_spread": round(spread["device_packed"], 4),
               "host_rounds_us": [round(t, 1) for t in times["host"]], "device_rounds_us": [round(t, 1) for t in times["device"]],
               "device_packed_rounds_us": [round(t, 1) for t in times["device_packed"]],
               "speedup": round(best["host"] / best["device"], 2), "bit_identical": bool(same)}
        lines.append(json.dumps(rec))
        rows.append(f"| {B:2d} | {rec['targets']:4d} | {rec['max_targets']:3d} | {best['host']:9.1f} ({100 * spread['host']:4.1f} %) | "
                    f"{best['device']:9.1f} ({100 * spread['device']:4.1f} %) | "
                    f"{best['device_packed']:9.1f} ({100 * spread['device_packed']:4.1f} %) | {rec['speedup']:5.2f}x | {same} |")
        print(rows[-1], flush=True)
    if args.profile_case is not None:
        return
    head = ["| B | targets | most per image | host matcher us / step (spread) | device matcher us / step (spread) | "
            "device matcher, targets packed beforehand | host / device | same bits |", "|---|---|---|---|---|---|---|---|"]
    text = "\n".join(head + rows) + "\n\n" + "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# tools/bench_detection_tail.py --assignment both on {dev}: the HIP detection tail (decoder + matcher + criterion,\n"
                    f"# forward and backward, from the transformer output [B, {N}, {D}] to its gradient; Q = {Q}, C = {C}) with the\n"
                    "# assignment solved by scipy on the host after a copy of the cost blocks, against the same tail with mv_det_match\n"
                    "# (targets packed inside every step, as a training step does, or once beforehand);\n"
                    f"# wall clock per step ending in a device synchronise, best of {MATCH_ROUNDS} alternating rounds of {MATCH_ITERS} steps;\n"
                    "# spread = slowest / fastest round - 1.  same bits: all five criterion values and the gradient of x.\n")
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--assignment", choices=("host", "device", "both"), default="host")
    ap.add_argument("--profile-case", type=int, choices=range(len(MATCH_CASES)))
    args = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    if args.assignment == "both":
        return compare_assignments(args, dev)
    gen = torch.Generator().manual_seed(0)
    rows, lines = [], []
    for B in (2, 64):
        x, dec, targets = make_case(B, gen)
        arms = {"hip": hip_arm(x, dec, targets, args.assignment), "torch": torch_arm(x, dec, targets)}
        a = arms["hip"]()
        gx = x.grad.clone()
        b = arms["torch"]()
        agree = max(abs(float(a[k].detach()) - float(b[k].detach())) / max(1.0, abs(float(b[k].detach()))) for k in a)
        agree = max(agree, float((gx - x.grad).abs().max() / x.grad.abs().max()))
        times = {k: [] for k in arms}
        for _ in range(ROUNDS):
            for k, fn in arms.items():                       # arms alternate inside a round
                times[k].append(timeit(fn, ITERS))
        best = {k: min(v) for k, v in times.items()}
        spread = {k: max(v) / min(v) - 1 for k, v in times.items()}
        rec = {"B": B, "N": N, "D": D, "Q": Q, "C": C, "targets": sum(len(t["labels"]) for t in targets), "device": dev,
               "rounds": ROUNDS, "iters": ITERS, "hip_us": round(best["hip"], 1), "torch_us": round(best["torch"], 1),
               "hip_spread": round(spread["hip"], 4), "torch_spread": round(spread["torch"], 4),
               "speedup": round(best["torch"] / best["hip"], 2), "max_rel_difference": float(f"{agree:.3e}")}
        lines.append(json.dumps(rec))
        rows.append(f"| {B:2d} | {rec['targets']:4d} | {best['hip']:9.1f} ({100 * spread['hip']:4.1f} %) | "
                    f"{best['torch']:9.1f} ({100 * spread['torch']:4.1f} %) | {rec['speedup']:5.2f}x | {agree:.1e} |")
        print(rows[-1], flush=True)
    head = ["| B | targets | HIP tail us / step (spread) | torch composition us / step (spread) | torch / HIP | max rel difference |",
            "|---|---|---|---|---|---|"]
    text = "\n".join(head + rows) + "\n\n" + "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# tools/bench_detection_tail.py on {dev}: decoder + matcher + criterion, forward and backward, from the\n"
                    f"# transformer output [B, {N}, {D}] to its gradient; Q = {Q}, C = {C}, 1..30 targets per image; wall clock per step\n"
                    f"# (host work and the matcher's synchronisation included), best of {ROUNDS} alternating rounds of {ITERS} steps;\n"
                    "# spread = slowest / fastest round - 1.  torch composition = the reference's arithmetic on the same device.\n")
            f.write(text)


if __name__ == "__main__":
    main()
