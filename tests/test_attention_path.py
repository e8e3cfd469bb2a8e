"""CPU: the one place an attention kernel family is chosen (``ops.attention_path``), the pairing of forward and backward wrappers
behind ``ops.attention_forward`` / ``ops.attention_backward`` as ``functional.attention_core`` and the fused attention block drive
them, the agreement of the Python length caps with the argument checks of the built library, and -- per kernel family -- the
``*_supported`` predicates at their caps and under the A/B switch, the bindings of the key-tiled entry points, the argument checks
that run before any device work (the 64-wide families; tests/test_attention_dh_dispatch.py has the widths 32 and 128)."""
import itertools
from contextlib import nullcontext

import pytest
import torch

from test_attention_short import MV_ERR_ALIGN, MV_ERR_SHAPE, MV_ERR_UNSUPPORTED, MV_OK

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture
def ops(monkeypatch):
    from myrtle_vision.hip import ops as _ops
    monkeypatch.setattr(_ops, "ATTN_LONG", True)
    return _ops


# ------------------------------------------------------------------------------------------------------------
# the truth table
# ------------------------------------------------------------------------------------------------------------
def expected_path(dtype, dh, N, need_grad, half_ok, hook, long_on, scope):
    """The three if / elif chains this function replaced (functional.attention_core and the two branches of the attention block),
    written out per (dtype, head width) band with literal caps."""
    if hook:
        return "probs"
    if dtype == BF16:
        if dh == 64:
            return "bf16" if N <= (8192 if long_on else 320) else "probs"
        if dh in (32, 128):
            return "bf16_dh" if long_on and N <= 8192 else "probs"
        return "probs"
    if dh != 64:                                            # fp32 q/k/v: only 64-wide heads have fused kernels
        return "probs"
    if half_ok and scope == 4 and N <= (8192 if long_on else 288):
        return "f16"
    if N <= (8192 if long_on else 272):
        return "f32" if need_grad else "f32_eval"
    return "probs"


def test_attention_path_truth_table(ops, monkeypatch):
    assert (ops.ATTN_BF16, ops.ATTN_BF16_DH, ops.ATTN_F16, ops.ATTN_F32, ops.ATTN_F32_EVAL, ops.ATTN_PROBS) == \
        ("bf16", "bf16_dh", "f16", "f32", "f32_eval", "probs")
    checked = 0
    for long_on, scope in itertools.product((True, False), (3, 4, 6)):
        monkeypatch.setattr(ops, "ATTN_LONG", long_on)
        with ops.segments(scope):
            for dtype, dh, N, need_grad, half_ok, hook in itertools.product(
                    (BF16, F32), (32, 48, 64, 128), (1, 208, 272, 273, 288, 289, 320, 321, 8192, 8193),
                    (False, True), (False, True), (False, True)):
                got = ops.attention_path(dtype, N, dh, need_grad=need_grad, half_ok=half_ok, hook=hook)
                want = expected_path(dtype, dh, N, need_grad, half_ok, hook, long_on, scope)
                assert got == want, (dtype, dh, N, need_grad, half_ok, hook, long_on, scope)
                checked += 1
    assert checked == 2 * 3 * 2 * 4 * 10 * 2 * 2 * 2


def test_attention_path_defaults_are_the_attention_core_call(ops):
    with ops.segments(4):                                   # attention_core never takes the half path, even in a bf16x3h scope
        assert ops.attention_path(F32, 197, 64, need_grad=True) == "f32"
        assert ops.attention_path(F32, 197, 64, need_grad=True, half_ok=True) == "f16"


def test_backward_refuses_what_a_path_does_not_do(ops):
    t = torch.zeros(1)
    for path in ("f32", "probs"):
        with pytest.raises(AssertionError):
            ops.attention_backward(path, t, t, t, t, 1, 1, 1, 64, 1.0, colsum=t)
    for path in ("bf16", "bf16_dh", "f32", "probs"):
        with pytest.raises(AssertionError):
            ops.attention_backward(path, t, t, t, t, 1, 1, 1, 64, 1.0, split=True)
    with pytest.raises(ValueError):
        ops.attention_backward("f32_eval", t, t, t, None, 1, 1, 1, 64, 1.0)
    with pytest.raises(ValueError):
        ops.attention_forward("nope", t, 1, 1, 1, 64, 1.0)
    assert ops.ATTN_COLSUM_PATHS == ("bf16", "bf16_dh", "f16")


# ------------------------------------------------------------------------------------------------------------
# forward / backward pairing, on recorders in place of every public wrapper (no device)
# ------------------------------------------------------------------------------------------------------------
PARTNER = {                                                  # forward wrapper(s) of a path -> its backward wrapper
    ("attention_fwd",): "attention_bwd",
    ("attention_fwd_dh",): "attention_bwd_dh",
    ("attention_fwd_f16",): "attention_bwd_f16",
    ("attention_fwd_f32_lse",): "attention_bwd_f32_fused",
    ("attention_probs_fp32", "attention_pv_fp32"): "attention_bwd_fp32",
    ("attention_fwd_f32",): None,
}
FILLS_COLSUM = {"attention_bwd", "attention_bwd_dh", "attention_bwd_f16"}


@pytest.fixture
def recorded(ops, monkeypatch):
    """Every public attention wrapper of ``ops`` replaced by a recorder that returns CPU tensors of the right shapes and dtypes;
    ``calls`` lists (wrapper, colsum given, split) in order."""
    calls = []

    def fwd(name, out_dtype, lse=True):
        def run(qkv, B, N, H, *rest, **kw):
            dh = rest[0] if name.endswith("_dh") else 64
            calls.append((name, False, False))
            out = torch.zeros(B, N, H * dh, dtype=out_dtype)
            return (out, torch.zeros(B, H, N)) if lse and kw.get("lse", True) else out
        return run

    def bwd(name, dq_dtype=None):
        def run(qkv, out, dout, lse, B, N, H, *rest, split=False, colsum=None):
            assert out.shape[:2] == dout.shape[:2] == (B, N) and lse.shape == (B, H, N) and dout.dtype == out.dtype
            calls.append((name, colsum is not None, split))
            if split:
                return torch.ones(B * N, ops.current_segments() * qkv.shape[2], dtype=BF16)
            return torch.ones(qkv.shape, dtype=dq_dtype or qkv.dtype)
        return run

    def probs(qkv, B, N, H, dh, scale):
        assert qkv.dtype == F32
        calls.append(("attention_probs_fp32", False, False))
        return torch.zeros(B, H, N, N)

    def pv(p, qkv, B, N, H, dh):
        assert p.shape == (B, H, N, N) and qkv.dtype == F32
        calls.append(("attention_pv_fp32", False, False))
        return torch.zeros(B, N, H * dh)

    def bwd_probs(p, qkv, dout, B, N, H, dh, scale):
        assert p.shape == (B, H, N, N) and qkv.dtype == dout.dtype == F32
        calls.append(("attention_bwd_fp32", False, False))
        return torch.ones_like(qkv)

    table = {"attention_probs_fp32": probs, "attention_pv_fp32": pv, "attention_bwd_fp32": bwd_probs,
             "attention_fwd_f32": fwd("attention_fwd_f32", F32, lse=False), "attention_bwd_f16": bwd("attention_bwd_f16", F32),
             "attention_bwd_long_f16": bwd("attention_bwd_long_f16", F32)}
    for name in ("attention_fwd", "attention_fwd_long", "attention_fwd_dh"):
        table[name] = fwd(name, BF16)
    for name in ("attention_fwd_f16", "attention_fwd_long_f16", "attention_fwd_f32_lse", "attention_fwd_long_f32"):
        table[name] = fwd(name, F32)
    for name in ("attention_fwd_f32_q8", "attention_fwd_long_f32_q8"):
        table[name] = fwd(name, torch.int8, lse=False)
    for name in ("attention_bwd", "attention_bwd_long", "attention_bwd_dh", "attention_bwd_f32_fused", "attention_bwd_long_f32"):
        table[name] = bwd(name)
    public = {n for n in dir(ops) if n.startswith("attention_") and not n.endswith("_supported")}
    assert set(table) == public - {"attention_path", "attention_forward", "attention_backward"}
    for name, fn in table.items():
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(ops, "cast", lambda src, dtype: src.to(dtype))
    return calls


def check_pairing(calls, want_fwd, colsum, split=False):
    names = [c[0] for c in calls]
    n = len(want_fwd)
    assert tuple(names[:n]) == want_fwd
    partner = PARTNER[want_fwd]
    assert names[n:] == ([partner] if partner else [])
    if partner:
        assert calls[n][1:] == (colsum, split)
        assert colsum <= (partner in FILLS_COLSUM)


CORE_CASES = [      # dtype, dh, N, ATTN_LONG, requires_grad -> forward wrapper(s)
    (BF16, 64, 17, True, True, ("attention_fwd",)),
    (BF16, 64, 321, True, True, ("attention_fwd",)),
    (BF16, 32, 17, True, True, ("attention_fwd_dh",)),
    (BF16, 128, 17, True, True, ("attention_fwd_dh",)),
    (F32, 64, 17, True, True, ("attention_fwd_f32_lse",)),
    (F32, 64, 273, True, True, ("attention_fwd_f32_lse",)),
    (F32, 64, 17, True, False, ("attention_fwd_f32",)),
]


@pytest.mark.parametrize("case", CORE_CASES, ids=lambda c: f"{str(c[0])[6:]}-dh{c[1]}-N{c[2]}-grad{int(c[4])}")
@pytest.mark.parametrize("scope", [6, 4])
def test_attention_core_pairs_forward_and_backward(ops, recorded, monkeypatch, case, scope):
    from myrtle_vision.hip import functional as F
    dtype, dh, N, long_on, grad, want_fwd = case
    monkeypatch.setattr(ops, "ATTN_LONG", long_on)
    qkv = torch.zeros(2, N, 3 * 2 * dh, dtype=dtype, requires_grad=grad)
    with ops.segments(scope):
        out = F.attention_core(qkv, 2, dh ** -0.5)
    assert out.shape == (2, N, 2 * dh) and out.dtype == dtype and out.requires_grad == grad
    if grad:
        out.backward(torch.ones(out.shape))                 # an fp32 dO: cast to bf16 for the bf16 kernels, kept for the fp32 ones
        assert bool((qkv.grad == 1).all())
    check_pairing(recorded, want_fwd, colsum=False)         # nothing downstream of attention_core reads column sums


@pytest.mark.parametrize("case", [(BF16, 48, 17, True, False), (BF16, 64, 321, False, False), (F32, 64, 273, False, False),
                                  (F32, 32, 17, True, False), (BF16, 64, 17, True, True), (F32, 64, 17, True, True)])
def test_attention_core_materialised_forward(ops, recorded, monkeypatch, case):
    """Forward only: the backward of this path lives in _AttentionProbs / _AttentionPV (they carry the hook) and goes to the
    library, not through ``ops.attention_backward``."""
    from myrtle_vision.hip import functional as F
    dtype, dh, N, long_on, hook = case
    monkeypatch.setattr(ops, "ATTN_LONG", long_on)
    seen = []
    qkv = torch.zeros(2, N, 3 * 2 * dh, dtype=dtype)
    out = F.attention_core(qkv, 2, dh ** -0.5, probs_hook=(lambda p: seen.append(p.shape) or p) if hook else None)
    assert out.shape == (2, N, 2 * dh) and out.dtype == dtype
    assert [c[0] for c in recorded] == ["attention_probs_fp32", "attention_pv_fp32"]
    assert seen == ([(2, 2, N, N)] if hook else [])


@pytest.fixture
def block(ops, recorded, monkeypatch):
    """The Linear, LayerNorm, split and column-sum ops the attention block calls, as recorders too.  ``bias_from`` collects where
    to_qkv's bias gradient came from: "colsum" (the attention kernel's per-image sums), "split_ex" or "linear_dw"."""
    bias_from = []

    def layernorm_fwd(x, ldx, rows, dim, g, b, out_dtype, eps=1e-5):
        return torch.zeros(rows, dim, dtype=out_dtype), torch.zeros(rows), torch.ones(rows)

    def layernorm_fwd_split(x, ldx, rows, dim, g, b, eps=1e-5):
        return torch.zeros(rows, ops.current_segments() * dim, dtype=BF16), torch.zeros(rows), torch.ones(rows)

    def split_ex(x, rows, cols, *, colsum_out=None, **kw):
        if colsum_out is not None and cols == block.inner3:
            bias_from.append("split_ex")
        return torch.zeros(rows, ops.current_segments() * cols, dtype=BF16)

    def linear_dw(dy, x, M, N, K, *, want_bias=True, weight=None, bias=None, **kw):
        if N == block.inner3 and want_bias:
            bias_from.append("linear_dw")
        return torch.zeros(N, K), (torch.zeros(N) if want_bias else None)

    def colsum(x, rows, cols, ld, out):
        if cols == block.inner3:
            bias_from.append("colsum")
        return out.zero_()

    def layernorm_bwd(dy, x, ldx, gamma, mean, rstd, dx_add, dx, lddx, rows, dim, **kw):
        dx.zero_()
        return torch.zeros(dim), torch.zeros(dim)

    monkeypatch.setattr(ops, "layernorm_fwd", layernorm_fwd)
    monkeypatch.setattr(ops, "layernorm_fwd_split", layernorm_fwd_split)
    monkeypatch.setattr(ops, "layernorm_bwd", layernorm_bwd)
    monkeypatch.setattr(ops, "split_ex", split_ex)
    monkeypatch.setattr(ops, "nt_x6", lambda a6, w, which, M, out, **kw: out.zero_())
    monkeypatch.setattr(ops, "tn_x6", lambda dy6, x6, M, w: torch.zeros(w.shape))
    monkeypatch.setattr(ops, "linear_fwd", lambda x, M, K, w, b, out, ldc, **kw: out.zero_())
    monkeypatch.setattr(ops, "linear_dx", lambda dy, M, N, w, out, ldc, **kw: out.zero_())
    monkeypatch.setattr(ops, "linear_dw", linear_dw)
    monkeypatch.setattr(ops, "colsum", colsum)

    def block(prec, dh, T, x6=True, grad=True):
        from myrtle_vision.hip import functional as F
        H, B = 2, 2
        D = H * dh
        block.inner3 = 3 * D
        monkeypatch.setattr(ops, "x6_block_ok", lambda M, *dims: x6)
        F.chain_reset()
        p = [torch.zeros(s, requires_grad=grad) for s in ((D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,))]
        x = torch.zeros(B, T, D, requires_grad=grad)
        out = F.attn_block(x, *p, H, dh ** -0.5, prec)
        assert out.shape == x.shape and out.requires_grad == grad
        if grad:
            out.backward(torch.ones_like(out))
            assert x.grad is not None and all(t.grad is not None and t.grad.shape == t.shape for t in p)
        return bias_from
    return block


BLOCK_CASES = [     # precision, dh, T, split-operand branch, ATTN_LONG, gradients -> forward wrapper(s), where to_qkv's bias gradient comes from
    ("bf16", 64, 17, False, True, True, ("attention_fwd",), "colsum"),
    ("bf16", 64, 321, False, True, True, ("attention_fwd",), "colsum"),
    ("bf16", 32, 17, False, True, True, ("attention_fwd_dh",), "colsum"),
    ("bf16", 128, 17, False, True, True, ("attention_fwd_dh",), "colsum"),
    ("bf16", 48, 17, False, True, True, ("attention_probs_fp32", "attention_pv_fp32"), "linear_dw"),
    ("bf16", 64, 321, False, False, True, ("attention_probs_fp32", "attention_pv_fp32"), "linear_dw"),
    ("bf16x3h", 64, 17, True, True, True, ("attention_fwd_f16",), "colsum"),
    ("bf16x3h", 64, 289, True, True, True, ("attention_fwd_f16",), "colsum"),
    ("bf16x3h", 64, 289, True, False, True, ("attention_probs_fp32", "attention_pv_fp32"), "split_ex"),
    ("bf16x3h", 64, 17, False, True, True, ("attention_fwd_f32_lse",), "linear_dw"),   # the plain branch never takes half q/k/v
    ("fp32", 64, 17, True, True, True, ("attention_fwd_f32_lse",), "split_ex"),
    ("fp32", 64, 273, True, True, True, ("attention_fwd_f32_lse",), "split_ex"),
    ("bf16x3", 64, 17, True, True, True, ("attention_fwd_f32_lse",), "split_ex"),
    ("fp32", 64, 273, True, False, True, ("attention_probs_fp32", "attention_pv_fp32"), "split_ex"),
    ("fp32", 64, 17, False, True, True, ("attention_fwd_f32_lse",), "linear_dw"),
    ("fp32", 64, 273, False, False, True, ("attention_probs_fp32", "attention_pv_fp32"), "linear_dw"),
    ("fp32", 64, 17, True, True, False, ("attention_fwd_f32",), None),
    ("fp32", 64, 17, False, True, False, ("attention_fwd_f32",), None),
    ("bf16x3h", 64, 17, True, True, False, ("attention_fwd_f16",), None),               # half first, whatever the gradient
]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: f"{c[0]}-dh{c[1]}-T{c[2]}-x6{int(c[3])}-long{int(c[4])}-grad{int(c[5])}")
def test_attn_block_pairs_forward_and_backward(ops, recorded, block, monkeypatch, case):
    prec, dh, T, x6, long_on, grad, want_fwd, bias_src = case
    monkeypatch.setattr(ops, "ATTN_LONG", long_on)
    bias_from = block(prec, dh, T, x6=x6, grad=grad)
    if not grad:
        assert [c[0] for c in recorded] == list(want_fwd) and bias_from == []
        return
    check_pairing(recorded, want_fwd, colsum=bias_src == "colsum", split=want_fwd == ("attention_fwd_f16",))
    assert bias_from == [bias_src]                           # exactly one source: never both, never neither


# ------------------------------------------------------------------------------------------------------------
# the caps of ops.py against the argument checks of the library (built library, no device: B = 0 launches nothing)
# ------------------------------------------------------------------------------------------------------------
OK, SHAPE, UNSUPPORTED = MV_OK, MV_ERR_SHAPE, MV_ERR_UNSUPPORTED
ADDR = 1 << 20                                               # 16-byte aligned, never read: every entry returns at B == 0
INTS = {                                                     # the int arguments of each signature shape, in order
    "std": lambda N, dh: [0, N, 2],                         # B, N, H
    "nseg": lambda N, dh: [0, 0, N, 2],                     # nseg, B, N, H
    "q8": lambda N, dh: [0, N, 2, 0],                       # B, N, H, zero point
    "dh": lambda N, dh: [0, N, 2, dh],                      # B, N, H, dim_head
}
CAP_CASES = [       # entry point, its ints, the Python constant, the code one past it
    ("mv_attention_fwd", "std", "ATTN_SHORT_MAX_N", SHAPE),
    ("mv_attention_bwd", "std", "ATTN_SHORT_MAX_N", SHAPE),
    ("mv_attention_fwd_f16", "std", "ATTN_F16_SHORT_MAX_N", UNSUPPORTED),
    ("mv_attention_bwd_f16", "nseg", "ATTN_F16_SHORT_MAX_N", UNSUPPORTED),
    ("mv_attention_fwd_f32", "std", "ATTN_F32_SHORT_MAX_N", UNSUPPORTED),
    ("mv_attention_fwd_f32_lse", "std", "ATTN_F32_SHORT_MAX_N", UNSUPPORTED),
    ("mv_attention_fwd_f32_q8", "q8", "ATTN_F32_SHORT_MAX_N", UNSUPPORTED),
    ("mv_attention_bwd_f32", "std", "ATTN_F32_SHORT_MAX_N", UNSUPPORTED),
    ("mv_attention_fwd_long", "std", "ATTN_LONG_MAX_N", SHAPE),
    ("mv_attention_bwd_long", "std", "ATTN_LONG_MAX_N", SHAPE),
    ("mv_attention_fwd_long_f16", "std", "ATTN_LONG_MAX_N", SHAPE),
    ("mv_attention_bwd_long_f16", "nseg", "ATTN_LONG_MAX_N", SHAPE),
    ("mv_attention_fwd_long_f32", "std", "ATTN_LONG_MAX_N", UNSUPPORTED),
    ("mv_attention_fwd_long_f32_q8", "q8", "ATTN_LONG_MAX_N", UNSUPPORTED),
    ("mv_attention_bwd_long_f32", "std", "ATTN_LONG_MAX_N", UNSUPPORTED),
    ("mv_attention_fwd_dh", "dh", "ATTN_LONG_MAX_N", SHAPE),
    ("mv_attention_bwd_dh", "dh", "ATTN_LONG_MAX_N", SHAPE),
]


def probe(entry, ints, N, dh=32):
    """Call ``entry`` with B = 0, a dummy address for every pointer and a null stream: the argument checks run, nothing else."""
    from myrtle_vision.hip import lib
    kinds = lib.SIGNATURES[entry][0]
    assert kinds[-1] == "p"
    ints = INTS[ints](N, dh)
    assert kinds.count("i") == len(ints)
    floats = iter([0.125, 1.0])                              # scale, then the quantiser's scale where there is one
    ints = iter(ints)
    args = [ADDR if k == "p" else next(ints) if k == "i" else next(floats) for k in kinds[:-1]]
    return getattr(lib.lib(), entry)(*args, None)


@pytest.mark.parametrize("entry,ints,const,past", CAP_CASES, ids=[c[0] for c in CAP_CASES])
def test_length_caps_agree_with_the_library(ops, entry, ints, const, past):
    cap = getattr(ops, const)
    assert cap == {"ATTN_SHORT_MAX_N": 320, "ATTN_F16_SHORT_MAX_N": 288, "ATTN_F32_SHORT_MAX_N": 272, "ATTN_LONG_MAX_N": 8192}[const]
    assert probe(entry, ints, cap) == OK
    assert probe(entry, ints, cap + 1) == past


@pytest.mark.parametrize("entry", ["mv_attention_fwd_dh", "mv_attention_bwd_dh"])
def test_dh_widths_agree_with_the_library(ops, entry):
    assert ops.ATTN_DH_WIDTHS == (32, 128)
    for w in ops.ATTN_DH_WIDTHS:
        assert probe(entry, "dh", 197, dh=w) == OK
    assert probe(entry, "dh", 197, dh=48) == UNSUPPORTED
    assert probe(entry, "dh", 197, dh=64) == UNSUPPORTED       # 64 has entry points of its own


def test_the_prep_helper_keeps_the_shape_tools_call_it_with(ops):
    """tools/bench_attn_long.py times the half backward's memory pass on its own: ``ops._attention_bwd_prep_f16(out, dout, B, N, H)``."""
    import inspect
    assert list(inspect.signature(ops._attention_bwd_prep_f16).parameters) == ["out", "dout", "B", "N", "H"]


# ------------------------------------------------------------------------------------------------------------
# per family: the *_supported predicates, the bindings, the argument checks
# ------------------------------------------------------------------------------------------------------------
# family -> its predicate, the q/k/v dtype and head width it answers for, the segment scope it needs (half: the bf16x3h scope)
PREDICATE = {"bf16": ("attention_fused_supported", BF16, 64, None), "half": ("attention_f16_supported", F32, 64, 4),
             "fp32": ("attention_f32_fused_supported", F32, 64, None)}
FUSED_N = {"bf16": [1, 197, 257, 320, 321, 577, 785, 1025, 4097, 8192], "half": [1, 197, 257, 288, 289, 321, 577, 1025, 4097, 8192],
           "fp32": [1, 197, 272, 273, 577, 1025, 4097, 8192]}


def holds(ops, monkeypatch, rows):
    """rows of (ATTN_LONG, segment scope or None, predicate, dtype, N, head width, expected)"""
    for long_on, scope, pred, dtype, N, w, want in rows:
        monkeypatch.setattr(ops, "ATTN_LONG", long_on)
        with ops.segments(scope) if scope else nullcontext():
            assert bool(getattr(ops, pred)(dtype, N, w)) == want, (long_on, scope, pred, dtype, N, w)


@pytest.mark.parametrize("family,N", [(f, n) for f, ns in FUSED_N.items() for n in ns])
def test_attention_is_fused_up_to_the_cap(ops, monkeypatch, family, N):
    pred, dtype, w, scope = PREDICATE[family]
    holds(ops, monkeypatch, [(True, scope, pred, dtype, N, w, True)])


FUSED, F16, F32_FUSED = (PREDICATE[f][0] for f in ("bf16", "half", "fp32"))
# past the cap, another width, another dtype; then ATTN_LONG off, the A/B tools' materialised arm: the whole-head caps
LIMITS = {
    "bf16": [(True, None, FUSED, BF16, 8193, 64, False), (True, None, FUSED, BF16, 577, 32, False),
             (True, None, FUSED, F32, 577, 64, False),            # fp32 / bf16x3 / bf16x3h keep their paths
             (False, None, FUSED, BF16, 320, 64, True), (False, None, FUSED, BF16, 321, 64, False)],
    "half": [(True, 4, F16, F32, 8193, 64, False), (True, 4, F16, F32, 577, 32, False), (True, 4, F16, BF16, 577, 64, False),
             (False, 4, F16, F32, 288, 64, True), (False, 4, F16, F32, 289, 64, False), (False, 4, F16, F32, 577, 64, False)] +
            [(True, nseg, F16, F32, N, 64, False) for nseg in (3, 6) for N in (577, 197)],   # outside the half-attention scope
    "fp32": [(True, None, F32_FUSED, F32, 8193, 64, False), (True, None, F32_FUSED, F32, 577, 32, False),
             (True, None, F32_FUSED, BF16, 577, 64, False), (False, None, F32_FUSED, F32, 272, 64, True),
             (False, None, F32_FUSED, F32, 273, 64, False), (False, None, F32_FUSED, F32, 577, 64, False)],
}
# what a family's arrival left alone in the families before it
UNCHANGED = {
    "half": [(True, None, FUSED, F32, 577, 64, False), (True, 4, FUSED, F32, 577, 64, False)],
    "fp32": [(True, None, FUSED, BF16, 577, 64, True), (True, None, FUSED, F32, 577, 64, False), (True, 4, F16, F32, 577, 64, True),
             (True, 3, F16, F32, 577, 64, False), (True, 6, F16, F32, 577, 64, False),
             (False, None, FUSED, BF16, 320, 64, True), (False, None, FUSED, BF16, 321, 64, False),
             (False, 4, F16, F32, 288, 64, True), (False, 4, F16, F32, 289, 64, False)],
}


@pytest.mark.parametrize("family", list(LIMITS))
def test_attention_limits_and_the_ab_switch(ops, monkeypatch, family):
    holds(ops, monkeypatch, LIMITS[family])


@pytest.mark.parametrize("family", list(UNCHANGED))
def test_the_earlier_families_dispatch_is_unchanged(ops, monkeypatch, family):
    holds(ops, monkeypatch, UNCHANGED[family])


BOUND = {"bf16": {"mv_attention_fwd_long": None, "mv_attention_bwd_long": "ppppppp" "iii" "f" "p"},
         "half": {"mv_attention_fwd_long_f16": "ppp" "iii" "f" "p", "mv_attention_bwd_long_f16": "pppppp" "ipp" "iii" "f" "p"},
         "fp32": {"mv_attention_fwd_long_f32": "ppp" "iii" "f" "p", "mv_attention_fwd_long_f32_q8": "pp" "iii" "f" "f" "i" "p",
                  "mv_attention_bwd_long_f32": "pppppp" "iii" "f" "p"}}


@pytest.mark.parametrize("family", list(BOUND))
def test_key_tiled_entry_points_are_bound(family):
    from myrtle_vision.hip import lib
    handle = lib.lib()
    for name, kinds in BOUND[family].items():
        assert kinds is None or lib.SIGNATURES[name][0] == kinds
        assert getattr(handle, name) is not None


def test_long_half_entry_points_reject_bad_arguments():
    """Argument checks run before any device work: shapes past the cap, a bad segment count and misaligned or missing pointers."""
    from myrtle_vision.hip import lib
    L = lib.lib()
    a = ADDR                                          # never dereferenced (rejected first)
    assert L.mv_attention_fwd_long_f16(a, a, a, 1, 8193, 1, 0.125, None) == MV_ERR_SHAPE
    assert L.mv_attention_fwd_long_f16(a, a, a, 1, 0, 1, 0.125, None) == MV_ERR_SHAPE
    assert L.mv_attention_fwd_long_f16(a + 2, a, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    bwd = L.mv_attention_bwd_long_f16
    assert bwd(a, a, a, a, a, a, 0, None, None, 1, 8193, 1, 0.125, None) == MV_ERR_SHAPE
    assert bwd(a, a, a, a, a, a, 4, None, None, 1, 577, 1, 0.125, None) == MV_ERR_UNSUPPORTED
    assert bwd(a, a + 8, a, a, a, a, 3, None, None, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert bwd(a, a, a, a, a, a, 6, a, None, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN      # colsum without its workspace
    # B = 0 is a no-op that launches nothing
    assert L.mv_attention_fwd_long_f16(a, a, a, 0, 577, 1, 0.125, None) == MV_OK
    assert bwd(a, a, a, a, a, a, 0, a, a, 0, 577, 1, 0.125, None) == MV_OK


def test_long_fp32_entry_points_reject_bad_arguments():
    """Argument checks run before any device work: lengths past the cap, a bad quantiser, misaligned pointers and a missing lse or
    delta workspace."""
    from myrtle_vision.hip import lib
    L = lib.lib()
    a = ADDR                                          # never dereferenced (rejected first)
    fwd, q8, bwd = L.mv_attention_fwd_long_f32, L.mv_attention_fwd_long_f32_q8, L.mv_attention_bwd_long_f32
    assert fwd(a, a, a, 1, 8193, 1, 0.125, None) == MV_ERR_UNSUPPORTED
    assert fwd(a, a, None, 1, 8193, 1, 0.125, None) == MV_ERR_UNSUPPORTED
    assert fwd(a, a, a, 1, 0, 1, 0.125, None) == MV_ERR_SHAPE
    assert fwd(a, a, a, -1, 577, 1, 0.125, None) == MV_ERR_SHAPE
    assert fwd(a + 4, a, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert fwd(a, a + 8, None, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert q8(a, a, 1, 8193, 1, 0.125, 0.05, 128, None) == MV_ERR_UNSUPPORTED
    assert q8(a, a, 1, 577, 1, 0.125, 0.05, 256, None) == MV_ERR_UNSUPPORTED
    assert q8(a, a, 1, 577, 1, 0.125, 0.05, -1, None) == MV_ERR_UNSUPPORTED
    assert q8(a, a, 1, 577, 1, 0.125, 0.0, 128, None) == MV_ERR_SHAPE
    assert q8(a, a + 2, 1, 577, 1, 0.125, 0.05, 128, None) == MV_ERR_ALIGN
    assert bwd(a, a, a, a, a, a, 1, 8193, 1, 0.125, None) == MV_ERR_UNSUPPORTED
    assert bwd(a, a, a, a, a, a, 1, 0, 1, 0.125, None) == MV_ERR_SHAPE
    assert bwd(a, a + 4, a, a, a, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert bwd(a, a, a, a, a, a + 4, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert bwd(a, a, a, None, a, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN            # no lse
    assert bwd(a, a, a, a, None, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN            # no delta workspace
    # B = 0 is a no-op that launches nothing
    assert fwd(a, a, a, 0, 577, 1, 0.125, None) == MV_OK
    assert fwd(a, a, None, 0, 577, 1, 0.125, None) == MV_OK
    assert q8(a, a, 0, 577, 1, 0.125, 0.05, 128, None) == MV_OK
    assert bwd(a, a, a, a, a, a, 0, 577, 1, 0.125, None) == MV_OK
