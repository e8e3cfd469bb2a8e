"""A kernel's dynamic-LDS grant belongs to that kernel instantiation: a sibling of the same template launched just before must not
count as a raise for it (mv_launch / mv_grant_lds in csrc/mv_common.h).

A fresh process makes the calls of calls() in order.  Each is the first launch of its kernel in that process and follows a sibling
instantiation; each must return MV_OK and give the result its own test asks for -- the references, helpers and ceilings are those
of tests/test_attention_short.py, tests/attention_families.py and tests/test_hip_ops.py, imported from there.  The backward
calls take the forward's out and lse from the fp64 reference, so no forward kernel runs between two backward siblings.  The child
prints one line per call; the parent checks its exit status and counts the lines."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = H = 1


def calls():
    """[(label, function)] in launch order"""
    import torch
    import attention_families as AF
    import test_attention_short as S
    import test_hip_ops as G
    from myrtle_vision.hip import ops
    from myrtle_vision.hip.lib import check, lib

    cache, plain = {}, {}

    def inputs(family, N):
        """qkv, dout, and fp64 out, lse, dqkv: computed once per (family, N)"""
        if (family, N) not in cache:
            qkv, dout = S.random_inputs(family, "plain", B, N, H, seed=N)
            cache[family, N] = (qkv, dout) + S.exact_fp64(qkv, dout, H)
        return cache[family, N]

    def exact_forward(family, N):
        _, _, out, lse, _ = inputs(family, N)
        return {"out": out.to(torch.bfloat16 if family == "bf16" else torch.float32), "lse": lse.float()}

    def assert_grad(family, got, want):
        for a, b in zip(S.split_qkv(got.double().cpu(), H), S.split_qkv(want, H)):
            assert S.relmax(a, b) < S.CEIL[family][1]

    def fwd(family, N):
        qkv, _, want_out, want_lse, _ = inputs(family, N)
        r = S.run_fwd(S.Tight(), family, qkv, B, N, H)
        assert S.relmax(r["out"], want_out) < S.CEIL[family][0]
        assert float((r["lse"].double().cpu() - want_lse).abs().max()) < S.CEIL[family][2]

    def bwd(N, variant):
        qkv, dout, _, _, want = inputs("bf16", N)
        r = S.run_bwd(S.Tight(), "bf16", qkv, exact_forward("bf16", N), dout, B, N, H, variant)   # (forces, then 0 in a finally)
        assert_grad("bf16", r["dqkv"], want)

    def bwd_half(N, nseg):
        qkv, dout, _, _, want = inputs("half", N)
        r = S.run_bwd(S.Tight(), "half", qkv, exact_forward("half", N), dout, B, N, H, nseg)
        if nseg == 0:
            plain[N] = r["dqkv"]
            assert_grad("half", r["dqkv"], want)
        else:                                              # the pieces of exactly the plain form's fp32 values
            assert torch.equal(r["dqkv"], S.split_of(ops, plain[N], nseg))

    def long_f32():
        fam = AF.FAMILIES["fp32"]
        qkv, dout = AF.make(fam, ops, B, 65, H, seed=5)
        AF.check_against_fp64(fam, ops, qkv, dout, B, 65, H, long=True)

    def gemm_nt(variant):
        check(lib().mv_gemm_force_variant(variant, 0), "force_variant")
        try:
            G.test_gemm_nt_bias_f32_out(ops, 256, 256, 128)           # fp32 output, then bf16 output
        finally:
            check(lib().mv_gemm_force_variant(0, 0), "force_variant")

    def gemm_tn(variant):
        G.test_gemm_tn_every_variant(ops, variant, 512, 256, 256)

    def call(f, *a):
        return (f"{f.__name__}{a}", lambda: f(*a))

    return ([call(fwd, "bf16", 225), call(fwd, "bf16", 289), call(fwd, "half", 209)] +
            [call(bwd, 197, 0), call(bwd, 193, 5), call(bwd, 225, 0), call(bwd, 209, 8), call(bwd, 289, 0)] +
            [call(bwd_half, N, nseg) for N in (197, 209) for nseg in (0, 3, 6)] +
            [call(long_f32)] +
            [call(gemm_nt, 2568), call(gemm_nt, 2564), call(gemm_tn, 256)])


@pytest.mark.gpu
def test_first_launch_after_a_sibling_instantiation():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600)
    done = [ln for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert r.returncode == 0, (r.returncode, done[-1:], r.stderr[-3000:])
    assert len(done) == len(calls()), done


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "myrtle-vision_amd")):
        sys.path.insert(0, p)
    for label, f in calls():
        f()
        print("ok " + label, flush=True)
