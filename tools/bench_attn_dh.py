#!/usr/bin/env python3
"""The fused bf16 attention core for 32- and 128-wide heads against the materialised fp32 path it replaces, GPU.

H * dim_head = 768 (ViT-B's width): dim_head 32 with 24 heads and dim_head 128 with 6 heads, N in {197, 577, 1025}, batch 64.
Per case, alternating in one process, ROUNDS rounds: the fused forward and backward (ops.attention_fwd_dh / _bwd_dh, the backward
with its delta pass and the column sums, as functional._AttnBlock runs it) and the materialised path of functional._AttnBlock
(q, k, v cast to fp32, [B, H, N, N] probabilities, the fp32 products, the bf16 casts) forward and backward.  Reported: the best
round of each arm, and its spread (slowest round / fastest round - 1).  Algorithmic FLOP: forward 4 B H N^2 dh, backward
10 B H N^2 dh.

    python tools/bench_attn_dh.py [--out FILE]      (prints a table; FILE gets the same table and one JSON line per case)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "myrtle-vision_amd"))
import torch  # noqa: E402

from myrtle_vision.hip import ops  # noqa: E402

ROUNDS, BATCH = 3, 64
CASES = [(dh, 768 // dh, N) for dh in (32, 128) for N in (197, 577, 1025)]


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # us


def make_arms(B, N, H, dh, gen):
    scale = dh ** -0.5
    qkv = (torch.randn(B, N, 3 * H * dh, device="cuda", generator=gen) * 0.8).to(torch.bfloat16)
    dout = torch.randn(B, N, H * dh, device="cuda", generator=gen).to(torch.bfloat16)
    part = torch.empty(B, 3 * H * dh, device="cuda")
    out, lse = ops.attention_fwd_dh(qkv, B, N, H, dh, scale)

    def mat_fwd():
        q32 = ops.cast(qkv, torch.float32)
        probs = ops.attention_probs_fp32(q32, B, N, H, dh, scale)
        return ops.cast(ops.attention_pv_fp32(probs, q32, B, N, H, dh), torch.bfloat16), probs

    probs = mat_fwd()[1]

    def mat_bwd():
        return ops.cast(ops.attention_bwd_fp32(probs, ops.cast(qkv, torch.float32), ops.cast(dout, torch.float32), B, N, H, dh,
                                               scale), torch.bfloat16)

    return {"dh_fwd": lambda: ops.attention_fwd_dh(qkv, B, N, H, dh, scale),
            "dh_bwd": lambda: ops.attention_bwd_dh(qkv, out, dout, lse, B, N, H, dh, scale, colsum=part),
            "mat_fwd": mat_fwd, "mat_bwd": mat_bwd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows, lines = [], []
    for dh, H, N in CASES:
        arms = make_arms(BATCH, N, H, dh, gen)
        times = {k: [] for k in arms}
        for _ in range(ROUNDS):
            for k, fn in arms.items():                       # arms alternate inside a round
                times[k].append(timeit(fn, 50 if k.startswith("dh") else 10))
        best = {k: min(v) for k, v in times.items()}
        spread = {k: max(v) / min(v) - 1 for k, v in times.items()}
        flop = {"fwd": 4.0 * BATCH * H * N * N * dh, "bwd": 10.0 * BATCH * H * N * N * dh}
        rec = {"dim_head": dh, "H": H, "B": BATCH, "N": N, "device": dev, "rounds": ROUNDS}
        for k in arms:
            rec[k + "_us"] = round(best[k], 1)
            rec[k + "_spread"] = round(spread[k], 4)
            rec[k + "_tflops"] = round(flop[k[-3:]] / best[k] / 1e6, 1)
        rec["speedup_fwd"] = round(best["mat_fwd"] / best["dh_fwd"], 2)
        rec["speedup_bwd"] = round(best["mat_bwd"] / best["dh_bwd"], 2)
        lines.append(json.dumps(rec))
        cell = lambda k: f"{best[k]:8.1f} ({rec[k + '_tflops']:6.1f}, {100 * spread[k]:4.1f} %)"
        rows.append(f"| {dh:3d} | {H:2d} | {N:5d} | {cell('dh_fwd')} | {cell('dh_bwd')} | {cell('mat_fwd')} | {cell('mat_bwd')} | "
                    f"{rec['speedup_fwd']:5.2f}x | {rec['speedup_bwd']:5.2f}x |")
        print(rows[-1], flush=True)
        del arms
        torch.cuda.empty_cache()
    head = ["| dim_head | H | N | fused fwd us (TFLOP/s, spread) | fused bwd us (TFLOP/s, spread) | materialised fwd | materialised bwd "
            "| fwd speed-up | bwd speed-up |", "|---|---|---|---|---|---|---|---|---|"]
    text = "\n".join(head + rows) + "\n\n" + "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# tools/bench_attn_dh.py on {dev}, H * dim_head = 768, batch {BATCH}, best of {ROUNDS} alternating rounds;\n"
                    "# spread = slowest / fastest round - 1.  materialised = functional._AttnBlock's path for these widths before\n"
                    "# (ops.ATTN_LONG off)\n")
            f.write(text)


if __name__ == "__main__":
    main()
