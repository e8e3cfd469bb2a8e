"""Time stochastic depth (drop path): the two streaming kernels of csrc/drop_path.hip against their byte counts, and the ViT-B/16
batch-256 bf16 training step with ``drop_path_rate`` 0.1 against the same step with the rate at 0 (the launches of a model
without the feature).

    python tools/bench_drop_path.py [--rounds 15] [--reps 3] [--batch 256] [--out profiles/drop_path.txt]

The variants run in alternation in one process, so that drift and other people's work on the host land on all of them alike;
``step_rate_0_again`` shows the spread the comparison has to clear.  Every timing is device events around ``reps`` calls; the
medians of the rounds are reported.  Needs an MI355X: without one it fails."""
import argparse
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop_path.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_drop_path needs an MI355X: a timing taken anywhere else says nothing")
    from myrtle_vision.hip import ops
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.optim import AdamW, ParamArena

    dev = torch.device("cuda")
    B, T, D = args.batch, 197, 768
    P = B * T * D * 4                                              # bytes of one fp32 [B, T, D] tensor
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, T, D, device=dev, generator=gen)
    f = torch.randn(B, T, D, device=dev, generator=gen)
    out32, out16 = torch.empty_like(x), torch.empty(B, T, D, dtype=torch.bfloat16, device=dev)
    kept = torch.full((B,), 1.0 / 0.9, device=dev)
    mixed = kept.clone()
    mixed[::10] = 0.0                                              # a tenth of the samples dropped: their f is not read
    kernels = [("add_all_kept", lambda: ops.drop_path_add(x, f, kept), 3.0),
               ("add_tenth_dropped", lambda: ops.drop_path_add(x, f, mixed), 2.9),
               ("scale_f32_to_bf16", lambda: ops.row_scale(x, kept, out=out16), 1.5),
               ("scale_f32_to_f32", lambda: ops.row_scale(x, kept, out=out32), 2.0),
               ("add_all_kept_again", lambda: ops.drop_path_add(x, f, kept), 3.0)]
    kt = timed([(name, fn) for name, fn, _ in kernels], args.rounds, 10)
    f.copy_(x)                                                     # (f grew by repeated accumulation; nothing reads it below)

    img = torch.randn(B, 3, 224, 224, device=dev, generator=gen)
    labels = torch.randint(0, 45, (B,), device=dev, generator=gen)

    def make(rate):
        torch.manual_seed(0)
        vit = ViT(decoder="classification", image_size=224, patch_size=16, num_classes=45, dim=768, depth=12, heads=12, mlp_dim=3072,
                  precision="bf16", q_format="FP32", drop_path_rate=rate).to(dev).train()
        opt = AdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-5, weight_decay=0.05)

        def step():
            opt.zero_grad()
            cross_entropy(vit(img), labels).backward()
            opt.step()
        return step

    off, on = make(0.0), make(0.1)
    steps = [("step_rate_0", off), ("step_rate_0.1", on), ("step_rate_0_again", off)]
    st = timed(steps, args.rounds, args.reps)

    lines = [f"drop path on {torch.cuda.get_device_name(0)}; {args.rounds} rounds in alternation, device events, medians",
             f"streaming kernels over fp32 [{B}, {T}, {D}] (P = {P / 1e6:.0f} MB), 10 calls per timing",
             f"{'kernel':<22}{'median us':>11}{'min us':>10}{'max us':>10}{'bytes / P':>11}{'GB/s at median':>16}"]
    for name, _, per_p in kernels:
        t = kt[name]
        m = statistics.median(t)
        lines.append(f"{name:<22}{m:>11.1f}{min(t):>10.1f}{max(t):>10.1f}{per_p:>11.1f}{per_p * P / m / 1e3:>16.0f}")
    lines.append(f"ViT-B/16 bf16 training step (forward, cross entropy, backward, AdamW), batch {B}, {args.reps} steps per timing")
    lines.append(f"{'variant':<22}{'median ms':>11}{'min ms':>10}{'max ms':>10}")
    med = {}
    for name, _ in steps:
        t = [v / 1e3 for v in st[name]]
        med[name] = statistics.median(t)
        lines.append(f"{name:<22}{med[name]:>11.3f}{min(t):>10.3f}{max(t):>10.3f}")
    base = med["step_rate_0"]
    lines.append(f"step_rate_0_again / step_rate_0 = {med['step_rate_0_again'] / base:.4f} (the spread of the comparison)")
    lines.append(f"step_rate_0.1 / step_rate_0     = {med['step_rate_0.1'] / base:.4f} "
                 f"(+{med['step_rate_0.1'] - base:.3f} ms for 22 branches; by bytes 22 * 3.5 P = {22 * 3.5 * P / 1e9:.1f} GB)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
