#!/usr/bin/env python3
"""The key-tiled bf16 attention core (N > 320) against the materialised fp32 path it replaces, ViT-B heads (H = 12), GPU.

Per length, alternating in one process (best of ROUNDS; the JSON lines also carry each arm's spread, slowest round / fastest
round - 1): the long forward and backward (ops.attention_fwd_long / _bwd_long),
the materialised path of functional._AttnBlock (q, k, v cast to fp32, [B, H, N, N] probabilities, the fp32 products, the
bf16 casts) forward and backward, and at N = 257 the whole-head kernels (mv_attention_fwd / _bwd) that the long ones would
replace there -- the price of being general.  Algorithmic FLOP: forward 4 B H N^2 64, backward 10 B H N^2 64.
``--half``: the same for the half-operand core of precision "bf16x3h" (fp32 q/k/v cast to half, fp32 outputs): the key-tiled half
kernels (ops.attention_fwd_long_f16 / _bwd_long_f16, the backward with its dO prep pass and the column sums, as the block runs it;
the prep pass alone is timed as "prep")
against the materialised fp32 path of functional._AttnBlock's fp32 branch (no casts), and at N = 257 against mv_attention_fwd_f16 /
_bwd_f16.
``--f32``: the same for the exact-fp32 core of precisions "fp32" / "bf16x3": the key-tiled f32 kernels (ops.attention_fwd_long_f32
with its lse / _bwd_long_f32, the backward with its delta pass) against the same materialised fp32 path, and at N = 257 against the
whole-head fp32 kernels (mv_attention_fwd_f32_lse / mv_attention_bwd_f32).

    python tools/bench_attn_long.py [--half | --f32] [--out FILE]      (prints a table; FILE gets the same table and one JSON line per case)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "myrtle-vision_amd"))
import torch  # noqa: E402

from myrtle_vision.hip import ops  # noqa: E402

H, SCALE, ROUNDS = 12, 0.125, 3
CASES = [(64, 577), (32, 785), (32, 1025), (2, 4097), (64, 257)]


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


def materialised_fwd(qkv, B, N):
    q32 = ops.cast(qkv, torch.float32)
    probs = ops.attention_probs_fp32(q32, B, N, H, 64, SCALE)
    return ops.cast(ops.attention_pv_fp32(probs, q32, B, N, H, 64), torch.bfloat16), probs


def materialised_bwd(probs, qkv, dout, B, N):
    return ops.cast(ops.attention_bwd_fp32(probs, ops.cast(qkv, torch.float32), ops.cast(dout, torch.float32), B, N, H, 64, SCALE),
                    torch.bfloat16)


def bf16_arms(B, N, gen):
    qkv = (torch.randn(B, N, 3 * H * 64, device="cuda", generator=gen) * 0.8).to(torch.bfloat16)
    dout = torch.randn(B, N, H * 64, device="cuda", generator=gen).to(torch.bfloat16)
    out, lse = ops.attention_fwd_long(qkv, B, N, H, SCALE)
    arms = {
        "long_fwd": lambda: ops.attention_fwd_long(qkv, B, N, H, SCALE),
        "long_bwd": lambda: ops.attention_bwd_long(qkv, out, dout, lse, B, N, H, SCALE),
    }
    if N <= ops.ATTN_SHORT_MAX_N:
        sout, slse = ops.attention_fwd(qkv, B, N, H, SCALE)
        arms["short_fwd"] = lambda: ops.attention_fwd(qkv, B, N, H, SCALE)
        arms["short_bwd"] = lambda: ops.attention_bwd(qkv, sout, dout, slse, B, N, H, SCALE)
    else:
        mout, probs = materialised_fwd(qkv, B, N)
        arms["mat_fwd"] = lambda: materialised_fwd(qkv, B, N)
        arms["mat_bwd"] = lambda: materialised_bwd(probs, qkv, dout, B, N)
    return arms


def half_arms(B, N, gen):
    """The bf16x3h arms: half q/k/v (what to_qkv writes), fp32 dout; the materialised arm on the fp32 q/k/v of the fp32 branch."""
    q32 = torch.randn(B, N, 3 * H * 64, device="cuda", generator=gen) * 0.8
    q16 = ops.cast_f16(q32)
    dout = torch.randn(B, N, H * 64, device="cuda", generator=gen)
    part = torch.empty(B, 3 * H * 64, device="cuda")
    out, lse = ops.attention_fwd_long_f16(q16, B, N, H, SCALE)
    arms = {
        "long_fwd": lambda: ops.attention_fwd_long_f16(q16, B, N, H, SCALE),
        "long_bwd": lambda: ops.attention_bwd_long_f16(q16, out, dout, lse, B, N, H, SCALE, colsum=part),
        "prep": lambda: ops._attention_bwd_prep_f16(out, dout, B, N, H),      # the part of long_bwd that is a memory pass
    }
    if N <= ops.ATTN_F16_SHORT_MAX_N:
        sout, slse = ops.attention_fwd_f16(q16, B, N, H, SCALE)
        arms["short_fwd"] = lambda: ops.attention_fwd_f16(q16, B, N, H, SCALE)
        arms["short_bwd"] = lambda: ops.attention_bwd_f16(q16, sout, dout, slse, B, N, H, SCALE, colsum=part)
    else:
        probs = ops.attention_probs_fp32(q32, B, N, H, 64, SCALE)
        arms["mat_fwd"] = lambda: ops.attention_pv_fp32(ops.attention_probs_fp32(q32, B, N, H, 64, SCALE), q32, B, N, H, 64)
        arms["mat_bwd"] = lambda: ops.attention_bwd_fp32(probs, q32, dout, B, N, H, 64, SCALE)
    return arms


def f32_arms(B, N, gen):
    """The fp32 / bf16x3 arms: fp32 q/k/v and dout throughout."""
    q32 = torch.randn(B, N, 3 * H * 64, device="cuda", generator=gen) * 0.8
    dout = torch.randn(B, N, H * 64, device="cuda", generator=gen)
    out, lse = ops.attention_fwd_long_f32(q32, B, N, H, SCALE)
    arms = {
        "long_fwd": lambda: ops.attention_fwd_long_f32(q32, B, N, H, SCALE),
        "long_bwd": lambda: ops.attention_bwd_long_f32(q32, out, dout, lse, B, N, H, SCALE),
    }
    if N <= ops.ATTN_F32_SHORT_MAX_N:
        sout, slse = ops.attention_fwd_f32_lse(q32, B, N, H, SCALE)
        arms["short_fwd"] = lambda: ops.attention_fwd_f32_lse(q32, B, N, H, SCALE)
        arms["short_bwd"] = lambda: ops.attention_bwd_f32_fused(q32, sout, dout, slse, B, N, H, SCALE)
    else:
        probs = ops.attention_probs_fp32(q32, B, N, H, 64, SCALE)
        arms["mat_fwd"] = lambda: ops.attention_pv_fp32(ops.attention_probs_fp32(q32, B, N, H, 64, SCALE), q32, B, N, H, 64)
        arms["mat_bwd"] = lambda: ops.attention_bwd_fp32(probs, q32, dout, B, N, H, 64, SCALE)
    return arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    kind = ap.add_mutually_exclusive_group()
    kind.add_argument("--half", action="store_true", help="the half-operand core of bf16x3h instead of the bf16 one")
    kind.add_argument("--f32", action="store_true", help="the exact-fp32 core of fp32 / bf16x3 instead of the bf16 one")
    args = ap.parse_args()
    lines, rows = [], []
    dev = torch.cuda.get_device_name(0)
    short_cap = ops.ATTN_F16_SHORT_MAX_N if args.half else ops.ATTN_F32_SHORT_MAX_N if args.f32 else ops.ATTN_SHORT_MAX_N
    for B, N in CASES:
        gen = torch.Generator(device="cuda").manual_seed(N)
        iters = max(3, min(50, int(2e12 / (10.0 * B * H * N * N * 64) * 20)))
        arms = half_arms(B, N, gen) if args.half else f32_arms(B, N, gen) if args.f32 else bf16_arms(B, N, gen)
        times = {k: [] for k in arms}
        for _ in range(ROUNDS):
            for k, fn in arms.items():
                times[k].append(timeit(fn, iters))
        best = {k: min(v) for k, v in times.items()}
        fl_f, fl_b = 4.0 * B * H * N * N * 64, 10.0 * B * H * N * N * 64
        other = "short" if N <= short_cap else "mat"
        rec = {"B": B, "N": N, "H": H, "device": dev, "iters": iters, "rounds": ROUNDS}
        if args.half:
            rec["core"] = "half (bf16x3h)"
        elif args.f32:
            rec["core"] = "fp32 (fp32, bf16x3)"
        for k, us in best.items():
            rec[k + "_us"] = round(us, 1)
            rec[k + "_spread"] = round(max(times[k]) / us - 1, 4)      # slowest round / fastest round - 1
            if k == "prep":
                continue
            rec[k + "_tflops"] = round((fl_f if k.endswith("fwd") else fl_b) / us / 1e6, 1)
        rec["speedup_fwd_bwd"] = round((best[other + "_fwd"] + best[other + "_bwd"]) / (best["long_fwd"] + best["long_bwd"]), 2)
        lines.append(json.dumps(rec))
        rows.append(f"| {B:3d} | {N:5d} | {best['long_fwd']:9.1f} ({rec['long_fwd_tflops']:6.1f}) | "
                    f"{best['long_bwd']:9.1f} ({rec['long_bwd_tflops']:6.1f}) | {other:5s} | "
                    f"{best[other + '_fwd']:9.1f} ({rec[other + '_fwd_tflops']:6.1f}) | "
                    f"{best[other + '_bwd']:9.1f} ({rec[other + '_bwd_tflops']:6.1f}) | {rec['speedup_fwd_bwd']:5.2f}x |")
        print(rows[-1], flush=True)
        del arms
        torch.cuda.empty_cache()
    head = ["| B | N | long fwd us (TFLOP/s) | long bwd us (TFLOP/s) | vs | fwd us (TFLOP/s) | bwd us (TFLOP/s) | fwd+bwd speed-up |",
            "|---|---|---|---|---|---|---|---|"]
    text = "\n".join(head + rows) + "\n\n" + "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            if args.half:
                f.write(f"# tools/bench_attn_long.py --half on {dev}, ViT-B heads (H = 12), best of {ROUNDS} alternating rounds: the half-operand\n"
                        "# core of bf16x3h (long bwd includes the dO prep pass and the column sums)\n"
                        "# vs: mat = materialised fp32 path (functional._AttnBlock's fp32 branch above 288 tokens before), short = the\n"
                        "# whole-head half kernels\n")
            elif args.f32:
                f.write(f"# tools/bench_attn_long.py --f32 on {dev}, ViT-B heads (H = 12), best of {ROUNDS} alternating rounds: the exact-fp32\n"
                        "# core of fp32 / bf16x3 on the f32 matrix cores (long bwd includes the delta pass)\n"
                        "# vs: mat = materialised fp32 path (functional._AttnBlock above 272 tokens before), short = the whole-head fp32\n"
                        "# kernels\n")
            else:
                f.write(f"# tools/bench_attn_long.py on {dev}, ViT-B heads (H = 12), best of {ROUNDS} alternating rounds\n"
                        "# vs: mat = materialised fp32 path (functional._AttnBlock above 320 tokens before), short = the whole-head kernels\n")
            f.write(text)


if __name__ == "__main__":
    main()
