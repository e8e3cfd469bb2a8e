"""Time DeiT distillation: (a) ``mv_distill_loss`` forward + backward against the torch composition of the reference's
models/distill.py:142-151 on the same device, batch 256 at 45 and 1000 classes, and (b) the bf16 training step of the ViT-Ti student
at batch 256 with a ViT-B teacher against the same step without one (the launches of a run without ``distiller_config``).

    python tools/bench_distill.py [--rounds 15] [--reps 3] [--batch 256] [--out profiles/distill.txt]

The variants run in alternation in one process, so that drift and other people's work on the host land on all of them alike; every
baseline runs twice (``*_again``), which shows the spread the comparison has to clear.  Every timing is device events around
``reps`` calls; the medians of the rounds are reported.  No threshold: the figures are a record.  Needs an MI355X: without one it
fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "myrtle-vision_amd")]

import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402


def timed(series, rounds, reps):
    for _, fn in series:                                           # warm-up: code objects, occupancy queries, weight copies
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in series}
    for _ in range(rounds):
        for name, fn in series:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / reps)     # microseconds per call
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill needs an MI355X: a timing taken anywhere else says nothing")
    from myrtle_vision.hip.functional import cross_entropy, distill_loss
    from myrtle_vision.models.distill import DistillableViT, DistillWrapper
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.optim import AdamW, ParamArena

    dev = torch.device("cuda")
    B, T_, alpha = args.batch, 3.0, 0.5
    gen = torch.Generator(device=dev).manual_seed(0)

    def loss_pair(C):
        s = torch.randn(B, C, device=dev, generator=gen).requires_grad_(True)
        d = torch.randn(B, C, device=dev, generator=gen).requires_grad_(True)
        t = torch.randn(B, C, device=dev, generator=gen)
        y = torch.randint(0, C, (B,), device=dev, generator=gen)

        def hip():
            s.grad = d.grad = None
            distill_loss(s, d, t, y, T_, alpha).backward()

        def composed():                                            # reference distill.py:142-151, forward and autograd's backward
            s.grad = d.grad = None
            loss = TF.cross_entropy(s, y)
            kd = TF.kl_div(TF.log_softmax(d / T_, dim=-1), TF.softmax(t / T_, dim=-1).detach(), reduction="batchmean") * T_ ** 2
            (loss * alpha + kd * (1 - alpha)).backward()
        return [(f"torch_C{C}", composed), (f"mv_distill_loss_C{C}", hip), (f"torch_C{C}_again", composed)]

    losses = loss_pair(45) + loss_pair(1000)
    lt = timed(losses, args.rounds, 10)

    img = torch.randn(B, 3, 224, 224, device=dev, generator=gen)
    labels = torch.randint(0, 45, (B,), device=dev, generator=gen)
    tiny = dict(decoder="classification", image_size=224, patch_size=16, num_classes=45, dim=192, depth=12, heads=3, mlp_dim=768,
                precision="bf16", q_format="FP32")
    base = dict(tiny, dim=768, heads=12, mlp_dim=3072)

    def make(with_teacher):
        torch.manual_seed(0)
        if not with_teacher:
            vit = ViT(**tiny).to(dev).train()
            opt = AdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-5, weight_decay=0.05)

            def step():
                opt.zero_grad()
                cross_entropy(vit(img), labels).backward()
                opt.step()
            return step
        w = DistillWrapper(teacher=ViT(**base), student=DistillableViT(**tiny), temperature=T_, alpha=alpha).to(dev).train()
        opt = AdamW(ParamArena(w.named_parameters(), skip=w.unused_parameter_names()), lr=1e-5, weight_decay=0.05)

        def step():
            opt.zero_grad()
            w(img, labels).backward()
            opt.step()
        return step

    off, on = make(False), make(True)
    steps = [("step_vit_ti", off), ("step_vit_ti_teacher_b", on), ("step_vit_ti_again", off)]
    st = timed(steps, args.rounds, args.reps)

    lines = [f"DeiT distillation on {torch.cuda.get_device_name(0)}; {args.rounds} rounds in alternation, device events, medians",
             f"(a) loss forward + backward, batch {B}, T = {T_:g}, alpha = {alpha:g}, soft; 10 calls per timing",
             f"{'variant':<26}{'median us':>11}{'min us':>10}{'max us':>10}"]
    med = {}
    for name, _ in losses:
        t = lt[name]
        med[name] = statistics.median(t)
        lines.append(f"{name:<26}{med[name]:>11.1f}{min(t):>10.1f}{max(t):>10.1f}")
    for C in (45, 1000):
        lines.append(f"C = {C}: torch again / torch = {med[f'torch_C{C}_again'] / med[f'torch_C{C}']:.3f} (spread); "
                     f"torch / mv_distill_loss = {med[f'torch_C{C}'] / med[f'mv_distill_loss_C{C}']:.2f}x")
    lines.append(f"(b) bf16 training step (forward, loss, backward, AdamW), ViT-Ti/16 student, batch {B}, {args.reps} steps per timing; "
                 "the teacher is a frozen ViT-B/16 (forward only)")
    lines.append(f"{'variant':<26}{'median ms':>11}{'min ms':>10}{'max ms':>10}")
    for name, _ in steps:
        t = [v / 1e3 for v in st[name]]
        med[name] = statistics.median(t)
        lines.append(f"{name:<26}{med[name]:>11.3f}{min(t):>10.3f}{max(t):>10.3f}")
    b0 = med["step_vit_ti"]
    lines.append(f"step_vit_ti_again / step_vit_ti     = {med['step_vit_ti_again'] / b0:.4f} (the spread of the comparison)")
    lines.append(f"step_vit_ti_teacher_b / step_vit_ti = {med['step_vit_ti_teacher_b'] / b0:.4f} "
                 f"(+{med['step_vit_ti_teacher_b'] - b0:.3f} ms: the teacher's forward pass, one more token, the second head)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
