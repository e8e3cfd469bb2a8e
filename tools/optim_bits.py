#!/usr/bin/env python3
"""One `case array sha256` line per array after three steps of every optimizer on the work list, GPU: the bits of a build.

    python tools/optim_bits.py > bits.txt

Run it in two checkouts (it uses only the ``ops.*_table_step`` wrappers, ``build_items`` and ``build_item_tensors``) and compare the
two files: a refactor of the kernels must leave every line as it was.  The arena is the seeded edge arena of
``tests/optim_table_ref.py`` (lengths below 4, not a multiple of 4, exactly ITEM_MAX, ITEM_MAX + 1, several items per tensor) with a
learning-rate scale and a weight decay per tensor, some of them 0.  Cases:
    adamw   {EMA off, on} x {launch, device scalars} x {clip off, on}
    sgd     plain, momentum, nesterov, each without and with the EMA; nesterov with the EMA also on device scalars with the clip
    lamb    without and with the EMA; with the EMA also on device scalars with the clip
Arrays: p, every state array, ema, and for LAMB the workspace of per-item partial sums."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "myrtle-vision_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from myrtle_vision.hip import ops  # noqa: E402
from myrtle_vision.utils.optim import build_item_tensors, build_items  # noqa: E402
from optim_table_ref import edge_arena  # noqa: E402

STEPS, BETAS, EMA_DECAY = 3, (0.9, 0.999), 0.99
LRS = (1e-3, 7e-4, 3e-4)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("optim_bits needs the GPU the kernels are built for")
    dev = torch.device("cuda")
    sizes, offsets, total = edge_arena()
    scales = [(1.0, 0.75, 0.5625, 0.1)[i % 4] for i in range(len(sizes))]
    wds = [(0.05, 0.0, 0.01)[i % 3] for i in range(len(sizes))]
    off, length, seg, segments = build_items(offsets, sizes, list(zip(scales, wds)))
    item_tensor, first, count = build_item_tensors(sizes)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    items = (torch.tensor(off, dtype=torch.int64, device=dev), i32(length), i32(seg))
    item_tensor, tensor_range = i32(item_tensor), i32(list(zip(first, count))).reshape(-1, 2)
    seg_scale = torch.tensor([s for s, _ in segments], dtype=torch.float32, device=dev)
    seg_wd = torch.tensor([w for _, w in segments], dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(20240607)
    p0 = (torch.randn(total, generator=gen) * 0.05).to(dev)
    grads = [(torch.randn(total, generator=gen) * 1e-2).to(dev) for _ in range(STEPS)]
    clip = torch.tensor([0.37], dtype=torch.float32, device=dev)

    def run(case, kind, ema_on, device_scalars=False, clip_on=False, **extra):
        p, ema = p0.clone(), (p0.clone() if ema_on else None)
        state = {n: torch.zeros_like(p) for n in (("m", "v") if kind != "sgd" else ("buf",) if extra["momentum"] else ())}
        if kind == "lamb":
            state["workspace"] = ops.lamb_workspace(len(off), dev).zero_()
        for t in range(STEPS):
            lr, bc = LRS[t], [1.0 - b ** (t + 1) for b in BETAS]
            hyper = torch.tensor([lr] + bc, dtype=torch.float32, device=dev) if device_scalars else None
            kw = dict(lr=lr, grad_scale=0.5, clip_coef=clip if clip_on else None, hyper=hyper, ema=ema, ema_decay=EMA_DECAY if ema_on else 0.0)
            if kind == "adamw":
                ops.adamw_table_step(p, grads[t], state["m"], state["v"], items, seg_scale, seg_wd, beta1=BETAS[0], beta2=BETAS[1],
                                     eps=1e-8, step=t + 1, **kw)
            elif kind == "sgd":
                ops.sgd_table_step(p, grads[t], state.get("buf"), items, seg_scale, seg_wd, **extra, **kw)
            else:
                ops.lamb_table_step(p, grads[t], state["m"], state["v"], items, item_tensor, tensor_range, seg_scale, seg_wd,
                                    state["workspace"], beta1=BETAS[0], beta2=BETAS[1], eps=1e-6, step=t + 1, **kw)
        torch.cuda.synchronize()
        for name, a in [("p", p)] + list(state.items()) + ([("ema", ema)] if ema_on else []):
            raw = a.contiguous().view(torch.uint8).cpu().numpy().tobytes()
            print(f"{case} {name} {hashlib.sha256(raw).hexdigest()}", flush=True)

    on = lambda flag, word: word if flag else "no-" + word
    for ema_on in (False, True):
        for dev_sc in (False, True):
            for clip_on in (False, True):
                run(f"adamw/{on(ema_on, 'ema')}/{'device' if dev_sc else 'launch'}/{on(clip_on, 'clip')}", "adamw", ema_on, dev_sc, clip_on)
    for name, mom, nest in (("plain", 0.0, False), ("momentum", 0.9, False), ("nesterov", 0.9, True)):
        for ema_on in (False, True):
            run(f"sgd-{name}/{on(ema_on, 'ema')}", "sgd", ema_on, momentum=mom, nesterov=nest)
    run("sgd-nesterov/ema/device/clip", "sgd", True, True, True, momentum=0.9, nesterov=True)
    for ema_on in (False, True):
        run(f"lamb/{on(ema_on, 'ema')}", "lamb", ema_on)
    run("lamb/ema/device/clip", "lamb", True, True, True)


if __name__ == "__main__":
    main()
