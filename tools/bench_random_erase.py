"""Time Random Erasing: (a) the two launches of ``utils.random_erasing.RandomErasing`` against the torch loop a user would write
(boxes drawn on the host as timm draws them, one slice ``.normal_()`` per erased sample) on a [256, 3, 224, 224] batch at ``reprob``
0.25 and 1.0; (b) the ViT-B/16 batch-256 bf16 training step with the eraser in front of the model against the same step without
it; (c) the same two steps under ``GraphedTrainStep``.

    python tools/bench_random_erase.py [--rounds 15] [--reps 3] [--batch 256] [--out profiles/random_erase.txt]

The arms of a comparison run in alternation in one process, so that drift and other people's work on the host land on all of them
alike; every comparison has a second series of one arm (``..._again``) that shows the spread it has to clear.  Every timing is
device events around ``reps`` calls; the medians of the rounds are reported.  Needs an MI355X: without one it fails."""
import argparse
import math
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "myrtle-vision_amd")]

import torch  # noqa: E402


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


def torch_loop(x, probability, min_area=0.02, max_area=1 / 3, log_ratio=(math.log(0.3), math.log(1 / 0.3))):
    """timm's RandomErasing on a device batch, mode 'pixel', count 1: the host draws, one slice normal_() per erased sample."""
    B, _, H, W = x.shape
    for b in range(B):
        if random.random() > probability:
            continue
        for _ in range(10):
            target = random.uniform(min_area, max_area) * H * W
            ratio = math.exp(random.uniform(*log_ratio))
            h, w = int(round(math.sqrt(target * ratio))), int(round(math.sqrt(target / ratio)))
            if w < W and h < H:
                top, left = random.randint(0, H - h), random.randint(0, W - w)
                x[b, :, top:top + h, left:left + w].normal_()
                break
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "random_erase.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_random_erase needs an MI355X: a timing taken anywhere else says nothing")
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.graph import GraphedTrainStep
    from myrtle_vision.utils.optim import AdamW, ParamArena
    from myrtle_vision.utils.random_erasing import RandomErasing

    dev = torch.device("cuda")
    B = args.batch
    gen = torch.Generator(device=dev).manual_seed(0)
    random.seed(0)
    x = torch.randn(B, 3, 224, 224, device=dev, generator=gen)
    lines = [f"random erasing on {torch.cuda.get_device_name(0)}; {args.rounds} rounds in alternation, device events, medians",
             f"(a) erasing an fp32 [{B}, 3, 224, 224] batch in place, mode pixel, count 1, 10 calls per timing",
             f"{'variant':<26}{'median us':>11}{'min us':>10}{'max us':>10}{'erased MB / call':>18}"]
    for p in (0.25, 1.0):
        eraser = RandomErasing(probability=p)
        eraser.seed(1234)
        erased = []

        def ours():
            eraser(x)
            erased.append(eraser.last_boxes)
        series = [(f"hip_two_launches_p{p}", ours), (f"torch_loop_p{p}", lambda: torch_loop(x, p)), (f"hip_two_launches_p{p}_again", ours)]
        t = timed(series, args.rounds, 10)
        mb = sum(float((e[..., 2].long() * e[..., 3].long()).sum()) for e in erased) * 3 * 4 / len(erased) / 1e6   # h * w * Ch * 4 bytes
        med = {}
        for name, _ in series:
            med[name] = statistics.median(t[name])
            lines.append(f"{name:<26}{med[name]:>11.1f}{min(t[name]):>10.1f}{max(t[name]):>10.1f}"
                         + (f"{mb:>18.2f}" if name.startswith("hip") else f"{'':>18}"))
        base = med[f"hip_two_launches_p{p}"]
        lines.append(f"p = {p}: again / first = {med[f'hip_two_launches_p{p}_again'] / base:.3f} (the spread); torch loop / hip = "
                     f"{med[f'torch_loop_p{p}'] / base:.1f}x")

    img = torch.randn(B, 3, 224, 224, device=dev, generator=gen)
    labels = torch.randint(0, 45, (B,), device=dev, generator=gen)

    def make(probability):
        torch.manual_seed(0)
        vit = ViT(decoder="classification", image_size=224, patch_size=16, num_classes=45, dim=768, depth=12, heads=12, mlp_dim=3072,
                  precision="bf16", q_format="FP32").to(dev).train()
        opt = AdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-5, weight_decay=0.05)
        eraser = RandomErasing(probability=probability)
        eraser.seed(1234)
        loss_fn = lambda m, a, y: cross_entropy(m(eraser(a)), y)   # noqa: E731  (probability 0: the eraser returns its input)
        return vit, opt, loss_fn

    def eager(parts):
        vit, opt, loss_fn = parts
        buf = img.clone()

        def step():
            opt.zero_grad()
            loss_fn(vit, buf, labels).backward()
            opt.step()
        return step

    def graphed(parts):
        g = GraphedTrainStep(*parts, img, labels)
        return lambda: g(img, labels)

    for title, wrap in (("(b) ViT-B/16 bf16 training step (forward, cross entropy, backward, AdamW), eager", eager),
                        ("(c) the same step as one HIP graph (GraphedTrainStep)", graphed)):
        off, on = wrap(make(0.0)), wrap(make(0.25))
        steps = [("step_plain", off), ("step_reprob_0.25", on), ("step_plain_again", off)]
        st = timed(steps, args.rounds, args.reps)
        lines.append(f"{title}, batch {B}, {args.reps} steps per timing")
        lines.append(f"{'variant':<26}{'median ms':>11}{'min ms':>10}{'max ms':>10}")
        med = {}
        for name, _ in steps:
            t = [v / 1e3 for v in st[name]]
            med[name] = statistics.median(t)
            lines.append(f"{name:<26}{med[name]:>11.3f}{min(t):>10.3f}{max(t):>10.3f}")
        base = med["step_plain"]
        lines.append(f"step_plain_again / step_plain = {med['step_plain_again'] / base:.4f} (the spread of the comparison)")
        lines.append(f"step_reprob_0.25 / step_plain = {med['step_reprob_0.25'] / base:.4f} ({med['step_reprob_0.25'] - base:+.3f} ms)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
