"""Time the optimizer family over the ViT-B parameter arena (about 86 M fp32 elements): the one ``mv_adamw_table`` launch (measured
again here, in the same process), ``mv_sgd_table`` with plain and with Nesterov momentum, and the two launches of ``mv_lamb_table``
without and with the weight EMA.

    python tools/bench_optim_family.py [--rounds 15] [--reps 10] [--out profiles/optim_family.txt]

The variants run in alternation in one process (table, sgd, table again, nesterov, lamb, lamb_ema, ...), so that drift and other
people's work on the host land on all of them alike; the second table series shows the spread the comparison has to clear.  Every
timing is device events around ``reps`` steps.  There is no threshold: the expectation is the ratio of bytes per element (SGD 5/7 and
LAMB 10/7 of the table launch), printed beside each measured ratio.  Needs an MI355X: without one it fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "myrtle-vision_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from bench_optim_table import vit_base_arena  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_family.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_family needs an MI355X: a timing taken anywhere else says nothing")
    from myrtle_vision.hip import ops
    from myrtle_vision.utils.optim import build_item_tensors, build_items, layer_scales

    names, sizes, offsets, n_decay, total = vit_base_arena()
    scales = layer_scales(names, 0.75)
    wds = [0.0 if (o >= n_decay or n in ("pos_embedding", "cls_token")) else 0.05 for n, o in zip(names, offsets)]
    off, length, seg, segments = build_items(offsets, sizes, list(zip(scales, wds)))
    item_tensor, first, count = build_item_tensors(sizes)
    dev = torch.device("cuda")
    items = (torch.tensor(off, dtype=torch.int64, device=dev), torch.tensor(length, dtype=torch.int32, device=dev),
             torch.tensor(seg, dtype=torch.int32, device=dev))
    item_tensor = torch.tensor(item_tensor, dtype=torch.int32, device=dev)
    tensor_range = torch.tensor(list(zip(first, count)), dtype=torch.int32, device=dev)
    seg_scale = torch.tensor([s for s, _ in segments], dtype=torch.float32, device=dev)
    seg_wd = torch.tensor([w for _, w in segments], dtype=torch.float32, device=dev)
    ws = ops.lamb_workspace(len(off), dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(total, device=dev, generator=gen) * 0.02
    g = torch.randn(total, device=dev, generator=gen) * 1e-3
    m, v, buf, ema = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p), p.clone()
    adam = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=10)
    lamb = dict(adam, eps=1e-6)

    def table():
        ops.adamw_table_step(p, g, m, v, items, seg_scale, seg_wd, **adam)

    def sgd():
        ops.sgd_table_step(p, g, buf, items, seg_scale, seg_wd, lr=1e-4, momentum=0.9, nesterov=False)

    def nesterov():
        ops.sgd_table_step(p, g, buf, items, seg_scale, seg_wd, lr=1e-4, momentum=0.9, nesterov=True)

    def lamb_step():
        ops.lamb_table_step(p, g, m, v, items, item_tensor, tensor_range, seg_scale, seg_wd, ws, **lamb)

    def lamb_ema():
        ops.lamb_table_step(p, g, m, v, items, item_tensor, tensor_range, seg_scale, seg_wd, ws, ema=ema, ema_decay=0.9998, **lamb)

    series = [("table", table, 28), ("sgd", sgd, 20), ("table_again", table, 28), ("nesterov", nesterov, 20), ("lamb", lamb_step, 40),
              ("lamb_ema", lamb_ema, 48)]
    for _, fn, _ in series:                                        # warm-up: code objects, occupancy queries
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in series}
    for _ in range(args.rounds):
        for name, fn, _ in series:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / args.reps)        # microseconds per step
    elements = sum(sizes)
    tensor_items = sum(c * c for c in count)                       # item pairs phase 2 of LAMB reads again: count^2 per tensor
    lines = [f"optimizer family over the ViT-B arena: {elements} parameter elements in {len(sizes)} tensors ({total} with alignment "
             f"gaps), {len(off)} work items, {len(segments)} segments",
             f"device: {torch.cuda.get_device_name(0)}; {args.rounds} rounds in alternation, {args.reps} steps per timing, device events",
             f"lamb: its second launch reads {tensor_items} item pairs (16 B each, {tensor_items * 16 / 1e6:.1f} MB, from a "
             f"{len(off) * 16 / 1e3:.0f} kB workspace) on top of the per-element bytes below",
             f"{'variant':<14}{'median us':>11}{'min us':>10}{'max us':>10}{'B/element':>11}{'GB/s at median':>16}"
             f"{'/ table':>10}{'by bytes':>10}"]
    med = {name: statistics.median(times[name]) for name, _, _ in series}
    for name, _, bytes_per in series:
        t = times[name]
        lines.append(f"{name:<14}{med[name]:>11.1f}{min(t):>10.1f}{max(t):>10.1f}{bytes_per:>11d}"
                     f"{elements * bytes_per / med[name] / 1e3:>16.0f}{med[name] / med['table']:>10.4f}{bytes_per / 28:>10.4f}")
    lines.append(f"table_again / table = {med['table_again'] / med['table']:.4f} (the spread of the comparison)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
