#!/usr/bin/env python3
"""Byte-for-byte A/B of the key-tiled attention entry points between two BUILDS of the library, GPU.

    python tools/ab_attn_bits.py A.so B.so

Each library runs in a fresh child process (MV_LIB_PATH set, so nothing of the other build is ever loaded) on the same seeded inputs
and prints one SHA-256 per (case, tensor) over the raw bytes of out, lse, dqkv and colsum; the parent compares the two lists line
by line.  B = 2, H = 2 and the lengths at which a ring or a tail can go wrong:
    bf16 64-wide (attention_fwd_long / _bwd_long with colsum)              N = 1, 63, 64, 65, 127, 128, 129, 321, 577
    half 64-wide (attention_fwd_long_f16 / _bwd_long_f16 with colsum)      the same N; split False, and True under segments(3) and (6)
    width 32 (attention_fwd_dh / _bwd_dh, 256 rows per workgroup)          N = 1, 255, 256, 257, 577
    width 128                                                              N = 1, 127, 128, 129, 577
Exit status 0 when every tensor is identical, 1 otherwise."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H = 2, 2
N64 = (1, 63, 64, 65, 127, 128, 129, 321, 577)
NDH = {32: (1, 255, 256, 257, 577), 128: (1, 127, 128, 129, 577)}


def child():
    sys.path.insert(0, os.path.join(ROOT, "myrtle-vision_amd"))
    import torch
    from myrtle_vision.hip import ops

    def emit(case, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
            print(f"{case} {name} {tuple(t.shape)} {hashlib.sha256(raw).hexdigest()}", flush=True)

    def inputs(N, dh, seed):
        g = torch.Generator().manual_seed(seed)
        qkv = (torch.randn(B, N, 3 * H * dh, generator=g) * 0.8).cuda()
        dout = torch.randn(B, N, H * dh, generator=g).cuda()
        return qkv, dout

    for N in N64:
        qkv32, dout32 = inputs(N, 64, 1000 + N)
        qkv, dout = qkv32.to(torch.bfloat16), dout32.to(torch.bfloat16)
        out, lse = ops.attention_fwd_long(qkv, B, N, H, 0.125)
        colsum = torch.zeros(B, 3 * H * 64, device="cuda")
        dqkv = ops.attention_bwd_long(qkv, out, dout, lse, B, N, H, 0.125, colsum=colsum)
        emit(f"bf16/64 N={N}", out=out, lse=lse, dqkv=dqkv, colsum=colsum)

        q16 = ops.cast_f16(qkv32)
        out, lse = ops.attention_fwd_long_f16(q16, B, N, H, 0.125)
        colsum = torch.zeros(B, 3 * H * 64, device="cuda")
        dqkv = ops.attention_bwd_long_f16(q16, out, dout32, lse, B, N, H, 0.125, colsum=colsum)
        emit(f"half/64 N={N} fp32", out=out, lse=lse, dqkv=dqkv, colsum=colsum)
        for nseg in (3, 6):
            with ops.segments(nseg):
                colsum = torch.zeros(B, 3 * H * 64, device="cuda")
                dqkv = ops.attention_bwd_long_f16(q16, out, dout32, lse, B, N, H, 0.125, split=True, colsum=colsum)
            emit(f"half/64 N={N} split{nseg}", dqkv=dqkv, colsum=colsum)

    for dh, lengths in NDH.items():
        for N in lengths:
            qkv32, dout32 = inputs(N, dh, 2000 + 10 * N + dh)
            qkv, dout = qkv32.to(torch.bfloat16), dout32.to(torch.bfloat16)
            out, lse = ops.attention_fwd_dh(qkv, B, N, H, dh, dh ** -0.5)
            colsum = torch.zeros(B, 3 * H * dh, device="cuda")
            dqkv = ops.attention_bwd_dh(qkv, out, dout, lse, B, N, H, dh, dh ** -0.5, colsum=colsum)
            emit(f"bf16/{dh} N={N}", out=out, lse=lse, dqkv=dqkv, colsum=colsum)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    runs = []
    for path in sys.argv[1:]:
        env = dict(os.environ, MV_LIB_PATH=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True)
        if r.returncode != 0:                        # nothing more is started after a failed run
            sys.exit(f"{path}: exit status {r.returncode}\n{r.stdout}\n{r.stderr}")
        runs.append(r.stdout.splitlines())
    a, b = runs
    bad = 0
    for i in range(max(len(a), len(b))):
        la, lb = (a[i] if i < len(a) else "<missing>"), (b[i] if i < len(b) else "<missing>")
        same = la == lb
        bad += not same
        print(("same  " if same else "DIFF  ") + la + ("" if same else "\n      " + lb))
    print(f"{len(a)} tensors from {sys.argv[1]}, {len(b)} from {sys.argv[2]}: " + ("all identical" if not bad and a else f"{bad} differ"))
    sys.exit(0 if not bad and a else 1)


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main()
