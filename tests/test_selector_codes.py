"""CPU tests (no GPU): every entry point that turns a run-time selector (dtype code, op, role, nseg, epilogue, dim_head) into a
template argument answers a value outside its set with the code it always had, and launches nothing.

The library loads without a device and an entry point returns at its argument checks before any launch, so each call below ends on
the host.  All other arguments are valid (dummy, aligned addresses that are never read), so the selector alone decides the code.
The expected codes were recorded from the library as it was BEFORE the launches moved to mv_launch / mv_pick (the same table run
against that build); they are not taken from the code under test."""
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "myrtle_vision_hip.h")
OK, SHAPE, ALIGN, LAUNCH, UNSUPPORTED = 0, -1, -2, -3, -4
ADDR = 1 << 20                                               # 16-byte aligned, never read
BIG = 1 << 30                                                # workspace_bytes: more than any of these shapes needs


def _parameters():
    """entry point -> [(name, is_pointer)] from the header."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|long|size_t)\s+(mv_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        ps = [" ".join(p.split()) for p in m.group(2).split(",")]
        out[m.group(1)] = [(re.search(r"(\w+)$", p).group(1), "*" in p or "mv_stream_t" in p) for p in ps if p != "void"]
    return out


LN = dict(ldx=136, rows=5, dim=136, eps=1e-5)                # one workgroup's worth plus a ragged edge
LN_BWD = dict(ldx=136, rows=5, dim=136, lddx=136, accumulate=0, workspace_bytes=BIG, dy_dtype=0)
NT = dict(lda=256, ldb=256, ldc=64, M=64, N=64, K=256, ld_aux=64, aux_i=0, ld_out2=64, alpha=1.0)
GELU = 1                                                     # MV_EPI_GELU: bf16 output only, checked before anything is launched
F32 = dict(sa_m=64, sa_k=1, sa_b1=0, sa_b2=0, sb_k=64, sb_n=1, sb_b1=0, sb_b2=0, sc_m=64, sc_n=1, sc_b1=0, sc_b2=0, M=64, N=64, K=64,
           nb1=1, nb2=1, alpha=1.0, accumulate=0, ld_aux=64, aux_i=1, ld_out2=64)
ATT = dict(B=1, N=65, H=1, scale=0.125)                      # 65 tokens, one head
SPLIT = dict(ldx=136, ldo=136 * 6, seg=136, rows=5, cols=136)
SPLIT_EX = dict(ldx=136, ldh=136, rows=5, cols=136, workspace_bytes=BIG)
QUANT = dict(rows=5, cols=136, ld=144, scale=0.05, zero_point=128, qmin=0, qmax=255)

# entry point, its other (valid) arguments, the selector, the value outside its set, the code the library returned before this change
CASES = [
    ("mv_split3_bf16_ex", SPLIT_EX, "op", 3, SHAPE),
    ("mv_split2_bf16_ex", SPLIT_EX, "op", 3, SHAPE),
    ("mv_split3_bf16", SPLIT, "role", 2, SHAPE),
    ("mv_split2_bf16", SPLIT, "role", 2, SHAPE),
    ("mv_weight_split", dict(R=64, C=64), "nseg", 4, SHAPE),
    ("mv_layernorm_fwd_split", LN, "nseg", 4, UNSUPPORTED),
    ("mv_layernorm_bwd_split", LN_BWD, "nseg", 4, UNSUPPORTED),
    ("mv_attention_bwd_f16", ATT, "nseg", 4, UNSUPPORTED),
    ("mv_attention_bwd_long_f16", ATT, "nseg", 4, UNSUPPORTED),
    ("mv_layernorm_fwd", LN, "y_dtype", 7, UNSUPPORTED),
    ("mv_layernorm_bwd", LN_BWD, "dy_dtype", 7, UNSUPPORTED),
    ("mv_layernorm_bwd_split", dict(LN_BWD, nseg=3), "dy_dtype", 7, UNSUPPORTED),
    ("mv_patchify", dict(B=1, C=3, H=32, W=32, p=16), "out_dtype", 7, UNSUPPORTED),
    ("mv_embed_bwd_gather", dict(B=1, T=5, D=136), "dy_dtype", 7, UNSUPPORTED),
    ("mv_gather_patch_rows", dict(B=1, T=5, D=136), "dst_dtype", 7, UNSUPPORTED),
    ("mv_cast", dict(dst_dtype=0, n=680), "src_dtype", 7, UNSUPPORTED),
    ("mv_cast", dict(src_dtype=0, n=680), "dst_dtype", 7, UNSUPPORTED),
    ("mv_colsum", dict(ld=136, accumulate=0, rows=5, cols=136, workspace_bytes=BIG), "x_dtype", 7, UNSUPPORTED),
    ("mv_gelu_fwd", dict(n=680), "dtype", 7, UNSUPPORTED),
    ("mv_gelu_bwd", dict(n=680), "dtype", 7, UNSUPPORTED),
    ("mv_quant_affine_codes", dict(QUANT, pre_op=0), "x_dtype", 7, UNSUPPORTED),
    ("mv_quant_affine_i8", dict(rows=5, cols=136, ld=144, scale=0.05, zero_point=128, pre_op=0), "x_dtype", 7, UNSUPPORTED),
    ("mv_cross_entropy", dict(ld_dl=136, outer=5, C=136, inner=1, grad_scale=1.0), "dl_dtype", 7, UNSUPPORTED),
    ("mv_seg_ce_bwd", dict(ld_ds=8, grad_scale=1.0, B=1, C=8, h=4, w=4, H=16, W=16), "ds_dtype", 7, UNSUPPORTED),
    ("mv_dropout", dict(n=680, p=0.1, seed=1, offset=0), "dtype", 7, UNSUPPORTED),
    ("mv_gemm_nt_bf16", dict(NT, epilogue=GELU), "c_dtype", 7, UNSUPPORTED),
    ("mv_gemm_nt_bf16_scaled", dict(NT, epilogue=GELU), "c_dtype", 7, UNSUPPORTED),
    ("mv_gemm_nt_i8", dict(NT, epilogue=0, q_scale=0.05, q_zero_point=128), "c_dtype", 7, UNSUPPORTED),
    ("mv_gemm_f32", F32, "epilogue", 99, UNSUPPORTED),
    ("mv_gemm_nt_bf16", dict(NT, c_dtype=1), "epilogue", 99, UNSUPPORTED),
    ("mv_gemm_nt_bf16_scaled", dict(NT, c_dtype=1), "epilogue", 99, UNSUPPORTED),
    ("mv_gemm_nt_f16", NT, "epilogue", 99, UNSUPPORTED),
    ("mv_gemm_nt_i8", dict(NT, c_dtype=0, q_scale=0.05, q_zero_point=128), "epilogue", 99, UNSUPPORTED),
    ("mv_attention_fwd_dh", ATT, "dim_head", 64, UNSUPPORTED),
    ("mv_attention_bwd_dh", ATT, "dim_head", 64, UNSUPPORTED),
]


def call(entry, values, selector, value):
    from myrtle_vision.hip import lib
    params = _parameters()[entry]
    given = dict(values, **{selector: value})
    assert selector in [n for n, _ in params]
    args = [ADDR if ptr else given.pop(name) for name, ptr in params[:-1]]
    assert params[-1][0] == "stream" and set(given) <= {"alpha", "aux_i", "ld_out2", "ld_aux"}, (entry, given)   # shared dicts carry spares
    return getattr(lib.lib(), entry)(*args, None)


@pytest.mark.parametrize("entry,values,selector,value,code", CASES, ids=[f"{c[0]}-{c[2]}{c[3]}" for c in CASES])
def test_a_selector_outside_its_set_keeps_its_code(entry, values, selector, value, code):
    assert call(entry, values, selector, value) == code


def test_every_selector_of_the_header_is_in_the_table():
    """A new entry point with a dtype / op / role / nseg / epilogue / dim_head argument has to join CASES."""
    names = re.compile(r"^(\w*dtype|op|role|nseg|epilogue|dim_head)$")
    want = {(e, n) for e, ps in _parameters().items() for n, _ in ps if names.match(n)}
    assert want == {(c[0], c[2]) for c in CASES}, want ^ {(c[0], c[2]) for c in CASES}
