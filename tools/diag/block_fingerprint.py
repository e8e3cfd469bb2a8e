#!/usr/bin/env python3
"""A fingerprint of the fused transformer blocks: ``functional.attn_block`` / ``mlp_block`` forward and backward on tiny shapes, in every
arithmetic and on every path the block functions choose between.  Per case it prints the ordered trace of the ``ops`` calls the
functional layer makes (name, dtype and shape of every tensor argument, every int / float / string, every keyword name), a sha256 of
the full trace (the calls ``ops`` makes to its own public functions included: ``check`` names every launch) and a sha256 of ``out``,
``dx`` and every parameter gradient.  At the end, the kernel-timer records of one attn + mlp step in "bf16" and "fp32".
``hip/functional.py`` and ``hip/ops.py`` are read from MODULES (default: this tree's), everything else -- the library binding too --
from this tree: run the same file against a copy of another commit's two modules and diff the outputs.
``ops.current_segments`` (a getter, no launch) is left out of the trace.
usage: block_fingerprint.py [MODULES]"""
import hashlib, importlib.util, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "myrtle-vision_amd"))
import torch
import myrtle_vision.hip as hip

MODULES = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(hip.__file__)
for _name in ("ops", "functional"):
    _spec = importlib.util.spec_from_file_location(f"myrtle_vision.hip.{_name}", os.path.join(MODULES, _name + ".py"))
    _mod = importlib.util.module_from_spec(_spec)
    sys.modules[_spec.name] = _mod
    setattr(hip, _name, _mod)
    _spec.loader.exec_module(_mod)
    print(f"{_name}: {_mod.__file__} sha256 {hashlib.sha256(open(_mod.__file__, 'rb').read()).hexdigest()[:16]}", file=sys.stderr)
ops, F = hip.ops, hip.functional

SHORT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.uint8: "u8", torch.int32: "i32", torch.int64: "i64"}
lines, depth = [], [0]


def show(v):
    if torch.is_tensor(v):
        return f"{SHORT.get(v.dtype, v.dtype)}{list(v.shape)}"
    if isinstance(v, (bool, int, float, str)) or v is None:
        return repr(v)
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(show(e) for e in v) + ")"
    return str(v) if isinstance(v, torch.dtype) else type(v).__name__


def traced(name, fn):
    def run(*a, **kw):
        lines.append((depth[0], f"{name}(" + ", ".join([show(v) for v in a] + [f"{k}={show(v)}" for k, v in kw.items()]) + ")"))
        depth[0] += 1
        try:
            return fn(*a, **kw)
        finally:
            depth[0] -= 1
    return run


for _name, _fn in list(vars(ops).items()):
    if isinstance(_fn, types.FunctionType) and not _name.startswith("_") and _name != "current_segments":
        setattr(ops, _name, traced(_name, _fn))


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def params(gen, D, mlp):
    def leaf(*shape, scale=1.0, shift=0.0):
        return (torch.randn(*shape, generator=gen) * scale + shift).cuda().requires_grad_(True)
    attn = dict(g=leaf(D, scale=0.1, shift=1.0), b=leaf(D, scale=0.1), wqkv=leaf(3 * D, D, scale=D ** -0.5), bqkv=leaf(3 * D, scale=0.1),
                wo=leaf(D, D, scale=D ** -0.5), bo=leaf(D, scale=0.1))
    mlpp = dict(g=leaf(D, scale=0.1, shift=1.0), b=leaf(D, scale=0.1), w1=leaf(mlp, D, scale=D ** -0.5), b1=leaf(mlp, scale=0.1),
                w2=leaf(D, mlp, scale=mlp ** -0.5), b2=leaf(D, scale=0.1))
    return attn, mlpp


def case(block, prec, B, T, scaled, D=128, heads=2, mlp=256, mode=None):
    tag = f"{block} {prec} B{B} T{T} D{D} heads{heads} mlp{mlp} row_scale={'0,2,..' if scaled else None}" + (f" f32_gemm={mode}" if mode else "")
    gen = torch.Generator().manual_seed(1234)
    pa, pm = params(gen, D, mlp)
    x = torch.randn(B, T, D, generator=gen).cuda().requires_grad_(True)
    w = torch.randn(B, T, D, generator=gen).cuda()
    c = torch.tensor([0.0, 2.0] * (B // 2)).cuda() if scaled else None
    prev = ops.set_f32_gemm(mode) if mode else None
    del lines[:]
    try:
        F.chain_reset()
        out = x
        if block in ("attn", "chain"):
            out = F.attn_block(out, *pa.values(), heads, (D // heads) ** -0.5, prec, row_scale=c)
        if block in ("mlp", "chain"):
            out = F.mlp_block(out, *pm.values(), prec, row_scale=c)
        (out * w).sum().backward()
        torch.cuda.synchronize()
    finally:
        if mode:
            ops.set_f32_gemm(prev)
    print(f"== {tag}")
    for d, line in lines:
        if d == 0:
            print("  " + line)
    print(f"  full trace: {len(lines)} calls, sha256 {hashlib.sha256(chr(10).join(f'{d} {s}' for d, s in lines).encode()).hexdigest()[:32]}")
    grads = [("out", out), ("dx", x.grad)]
    grads += [(f"attn.{k}", v.grad) for k, v in pa.items() if block != "mlp"] + [(f"mlp.{k}", v.grad) for k, v in pm.items() if block != "attn"]
    for k, t in grads:
        print(f"  {digest(t)} {k}", flush=True)


class LoggingTimer(ops.KernelTimer):
    """Keeps the order of the records across names."""

    def __init__(self):
        super().__init__()
        self.log = []

    def end(self, name, start, flops, shape=None):
        super().end(name, start, flops, shape=shape)
        if start is not None:
            self.log.append((name, shape, flops))


def timer_records(prec, B=2, T=64, D=128, heads=2, mlp=256):
    gen = torch.Generator().manual_seed(1234)
    pa, pm = params(gen, D, mlp)
    x = torch.randn(B, T, D, generator=gen).cuda().requires_grad_(True)
    timer = LoggingTimer()
    ops.set_kernel_timer(timer)
    try:
        F.chain_reset()
        out = F.mlp_block(F.attn_block(x, *pa.values(), heads, (D // heads) ** -0.5, prec), *pm.values(), prec)
        out.sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    print(f"== kernel timer {prec} B{B} T{T}: summary keys {sorted(timer.summary())}")
    for rec in timer.log:
        print(f"  {rec!r},")


for block in ("attn", "mlp", "chain"):
    for prec in ("bf16", "fp32", "bf16x3", "bf16x3h"):
        for B, T in ((2, 17), (2, 64), (4, 64)):
            for scaled in (False, True):
                case(block, prec, B, T, scaled)
for block in ("attn", "chain"):                                    # dh = 48: the materialised probabilities and their casts
    for B, T in ((2, 17), (2, 64)):
        for scaled in (False, True):
            case(block, "bf16", B, T, scaled, D=96)
for block in ("attn", "mlp", "chain"):
    for scaled in (False, True):
        case(block, "fp32", 2, 64, scaled, D=1088, heads=17, mlp=1152)    # D > 1024: LayerNorm, then its split
        case(block, "fp32", 2, 64, scaled, mode="mfma")
for prec in ("bf16", "fp32"):
    timer_records(prec)
