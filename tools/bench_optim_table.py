"""Time the optimizer step over the ViT-B parameter arena (about 86 M fp32 elements): the two ``mv_adamw`` launches of the plain
optimizer against the one ``mv_adamw_table`` launch, without and with the weight EMA.

    python tools/bench_optim_table.py [--rounds 15] [--reps 10] [--out profiles/optim_table.txt]

The variants run in alternation in one process (two_launch, table, two_launch again, table_ema, ...), so that drift and other
people's work on the host land on all of them alike; the second two_launch series shows the spread the comparison has to clear.
Every timing is device events around ``reps`` steps.  Needs an MI355X: without one it fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "myrtle-vision_amd")]

import torch  # noqa: E402


def vit_base_arena():
    """ViT-B/16 classification (45 classes) laid out as ``ParamArena`` lays it out -> (names, sizes, offsets, n_decay, total)."""
    from myrtle_vision.models.vit import ViT
    with torch.device("meta"):
        vit = ViT(decoder="classification", image_size=224, patch_size=16, num_classes=45, dim=768, depth=12, heads=12, mlp_dim=3072)
    skip = set(vit.unused_parameter_names())
    named = [(n, p) for n, p in vit.named_parameters() if n not in skip]
    nd = lambda n, p: p.ndim <= 1 or n.endswith(".bias")
    order = [(n, p) for n, p in named if not nd(n, p)] + [(n, p) for n, p in named if nd(n, p)]
    n_decay_tensors = sum(not nd(n, p) for n, p in named)
    names, sizes, offsets, total = [], [], [], 0
    for n, p in order:
        names.append(n)
        sizes.append(p.numel())
        offsets.append(total)
        total += (p.numel() + 7) & ~7
    return names, sizes, offsets, offsets[n_decay_tensors], total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_table needs an MI355X: a timing taken anywhere else says nothing")
    from myrtle_vision.hip import ops
    from myrtle_vision.utils.optim import build_items, layer_scales

    names, sizes, offsets, n_decay, total = vit_base_arena()
    scales = layer_scales(names, 0.75)
    wds = [0.0 if (o >= n_decay or n in ("pos_embedding", "cls_token")) else 0.05 for n, o in zip(names, offsets)]
    off, length, seg, segments = build_items(offsets, sizes, list(zip(scales, wds)))
    dev = torch.device("cuda")
    items = (torch.tensor(off, dtype=torch.int64, device=dev), torch.tensor(length, dtype=torch.int32, device=dev),
             torch.tensor(seg, dtype=torch.int32, device=dev))
    seg_scale = torch.tensor([s for s, _ in segments], dtype=torch.float32, device=dev)
    seg_wd = torch.tensor([w for _, w in segments], dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(total, device=dev, generator=gen) * 0.02
    g = torch.randn(total, device=dev, generator=gen) * 1e-3
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    kw = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=10)

    def two_launch():
        for lo, hi, wd in ((0, n_decay, 0.05), (n_decay, total, 0.0)):
            ops.adamw_step(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], weight_decay=wd, **kw)

    def table():
        ops.adamw_table_step(p, g, m, v, items, seg_scale, seg_wd, **kw)

    def table_ema():
        ops.adamw_table_step(p, g, m, v, items, seg_scale, seg_wd, ema=ema, ema_decay=0.9998, **kw)

    series = [("two_launch", two_launch), ("table", table), ("two_launch_again", two_launch), ("table_ema", table_ema)]
    for _, fn in series:                                           # warm-up: code objects, occupancy queries
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in series}
    for _ in range(args.rounds):
        for name, fn in series:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / args.reps)        # microseconds per step
    elements = sum(sizes)
    lines = [f"optimizer step over the ViT-B arena: {elements} parameter elements in {len(sizes)} tensors ({total} with alignment "
             f"gaps), {len(off)} work items, {len(segments)} segments",
             f"device: {torch.cuda.get_device_name(0)}; {args.rounds} rounds in alternation, {args.reps} steps per timing, device events",
             f"{'variant':<18}{'median us':>11}{'min us':>10}{'max us':>10}{'B/element':>11}{'GB/s at median':>16}"]
    med = {}
    for (name, _), bytes_per in zip(series, (28, 28, 28, 36)):
        t = times[name]
        med[name] = statistics.median(t)
        lines.append(f"{name:<18}{med[name]:>11.1f}{min(t):>10.1f}{max(t):>10.1f}{bytes_per:>11d}"
                     f"{elements * bytes_per / med[name] / 1e3:>16.0f}")
    base = med["two_launch"]
    lines.append(f"two_launch_again / two_launch = {med['two_launch_again'] / base:.4f} (the spread of the comparison)")
    lines.append(f"table / two_launch            = {med['table'] / base:.4f}")
    lines.append(f"table_ema / two_launch        = {med['table_ema'] / base:.4f} (9/7 = {9 / 7:.4f} by bytes)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
