"""The key-tiled attention kernels at every block edge, called through the C ABI so that every length reaches them.

Five kernel sets: mv_attention_fwd_long / _bwd_long (64-wide bf16), mv_attention_fwd_long_f16 / _bwd_long_f16 with nseg 0 / 3 / 6
(64-wide half), mv_attention_fwd_long_f32 with lse, without, and _q8 / mv_attention_bwd_long_f32 (fp32), and mv_attention_fwd_dh /
_bwd_dh at widths 32 and 128 (csrc/attention_tiled.hip, csrc/attention_f32.hip).  Their geometry: 16-row MFMA tiles, 64-row
streamed blocks through a two-stage LDS ring (the parity of the block count decides which stage is live last), 128 rows per
workgroup (256 at width 32).  The battery of tests/test_attention_short.py, with its builders and helpers:

1. routing: softmax an exact permutation matrix -- which key reaches which query is pinned bit for bit.  A wrong key's block seen
   first leaves garbage in O and l that only the rescale by exp2(m_old - m_new) = 0 removes;
2. every length against fp64: the ceilings the per-family files hold these kernels to through ops' wrappers (BARS of
   tests/attention_families.py), the per-element forward and lse bounds re-derived for the online softmax (forward_bound /
   lse_bound, blocks > 0), and on two harder score distributions a backward bar of 2x the error of an fp64 emulation of the
   kernels' roundings (emulate, blockwise);
3. guard zones round every tensor, the workspaces included;
4. (image, head) independence: the workgroup index mixes query block, image and head;
5. zero gradient;
6. the API edges that launch nothing.

The CPU preconditions of the routing inputs at these lengths are cases of
tests/test_attention_short.py::test_routing_builder_gives_an_exact_permutation_softmax; the emulation's is the unmarked test below."""
import pytest
import torch

pytest.register_assert_rewrite("attention_families")   # its shared bodies assert: failures show the values
from attention_families import BARS
from test_attention_short import (DISTS, MV_ERR_ALIGN, MV_ERR_SHAPE, MV_ERR_UNSUPPORTED, MV_OK, OPERAND, Q8_SCALE, Q8_ZERO, SENTINEL,
                                  TILED_EDGES, TILED_EDGES_DH, Guarded, L, Tight, assert_routed_backward, assert_routed_forward,
                                  emulate, exact_fp64, forward_bound, heads, join_qkv, lse_bound, ops, ptr, random_inputs,  # noqa: F401
                                  rel_l2, routing_expected, routing_inputs, same_bits, slice_err, split_of, split_qkv, stream,
                                  unheads, untouched, zero_gradient_bound)

gpu = pytest.mark.gpu

SETS = ("long", "long_f16", "long_f32", "dh32", "dh128")
FAMILY = {"long": "bf16", "long_f16": "half", "long_f32": "fp32", "dh32": "bf16", "dh128": "bf16"}
WIDTH = {"long": 64, "long_f16": 64, "long_f32": 64, "dh32": 32, "dh128": 128}
LENGTHS = {"long": TILED_EDGES, "long_f16": TILED_EDGES, "long_f32": TILED_EDGES, "dh32": TILED_EDGES_DH[32],
           "dh128": TILED_EDGES_DH[128]}
EDGE_CLASS = [17, 65, 129, 257, 385, 513]          # one length per edge class: the harder distributions
GUARD_N = [1, 17, 65, 129, 257, 321, 513]
INDEPENDENT_N = {"long": [129, 385], "long_f16": [129, 385], "long_f32": [129, 385], "dh32": [129, 257], "dh128": [129, 385]}
# BARS: the whole-tensor L2 ceilings of each arithmetic, the ones tests/test_attention_long*.py and _dh.py apply: out, lse (absolute), grad
# (each of dq / dk / dv), colsum_own (against the sums of the returned dqkv), colsum64 (against fp64)


def set_lengths(lengths=None):
    return [(name, n) for name in SETS for n in LENGTHS[name] if lengths is None or n in lengths]


def scale_of(dh):
    return dh ** -0.5


def blocks_of(N):
    return (N + 63) // 64


def fwd_kinds(name):
    return ("lse", "plain", "q8") if name == "long_f32" else ("lse",)


def bwd_kinds(name):
    return (0, 3, 6) if name == "long_f16" else (0,)


# ================================================================== the raw entry points, on any allocation
def run_fwd(A, name, qkv, B, N, H, kind="lse"):
    """-> dict of outputs.  long_f32: kind "lse" | "plain" (lse == NULL) | "q8"."""
    family, dh = FAMILY[name], WIDTH[name]
    C, scale = H * dh, scale_of(dh)
    q = A.inp(qkv, OPERAND[family])
    r = {}
    if kind == "q8":
        r["codes"] = A.out((B, N, C), torch.int8)
        rc = L().mv_attention_fwd_long_f32_q8(ptr(q), ptr(r["codes"]), B, N, H, scale, Q8_SCALE, Q8_ZERO, stream())
    else:
        r["out"] = A.out((B, N, C), torch.bfloat16 if family == "bf16" else torch.float32)
        if kind == "lse":
            r["lse"] = A.out((B, H, N), torch.float32)
        args = (ptr(q), ptr(r["out"]), ptr(r.get("lse")), B, N, H)
        if name == "long":
            rc = L().mv_attention_fwd_long(*args, scale, stream())
        elif name == "long_f16":
            rc = L().mv_attention_fwd_long_f16(*args, scale, stream())
        elif name == "long_f32":
            rc = L().mv_attention_fwd_long_f32(*args, scale, stream())
        else:
            rc = L().mv_attention_fwd_dh(*args, dh, scale, stream())
    assert rc == MV_OK, (name, kind, N, rc)
    A.check()
    return r


def run_bwd(A, name, qkv, fw, dout, B, N, H, variant=0):
    """fw: the forward's out / lse.  -> dqkv and every other buffer the call writes: delta_ws and colsum (bf16 sets), delta_ws (fp32),
    the prep kernel's dout16 / delta / gscale, colsum and colsum_ws (half; variant = nseg: dqkv fp32, or the bf16 pieces)."""
    family, dh = FAMILY[name], WIDTH[name]
    C, scale = H * dh, scale_of(dh)
    q = A.inp(qkv, OPERAND[family])
    out, lse = A.inp(fw["out"]), A.inp(fw["lse"])
    r = {}
    if family == "bf16":
        d = A.inp(dout, torch.bfloat16)
        r["delta_ws"], r["dqkv"] = A.out((B, H, N), torch.float32), A.out((B, N, 3 * C), torch.bfloat16)
        r["colsum"] = A.out((B, 3 * C), torch.float32)
        args = (ptr(q), ptr(out), ptr(d), ptr(lse), ptr(r["delta_ws"]), ptr(r["dqkv"]), ptr(r["colsum"]), B, N, H)
        rc = L().mv_attention_bwd_long(*args, scale, stream()) if name == "long" else L().mv_attention_bwd_dh(*args, dh, scale, stream())
    elif family == "half":
        d = A.inp(dout, torch.float32)
        r["dout16"], r["delta"] = A.out((B, N, C), torch.float16), A.out((B, H, N), torch.float32)
        r["gscale"] = A.out((B * H,), torch.float32)
        rc = L().mv_attention_bwd_prep_f16(ptr(d), ptr(out), ptr(r["dout16"]), ptr(r["delta"]), ptr(r["gscale"]), B, N, H, stream())
        assert rc == MV_OK, (N, rc)
        A.check()
        d16, dl, gs = A.inp(r["dout16"]), A.inp(r["delta"]), A.inp(r["gscale"])
        r["colsum"], r["colsum_ws"] = A.out((B, 3 * C), torch.float32), A.out((B, (N + 127) // 128, 3 * C), torch.float32)
        r["dqkv"] = A.out((B * N, variant * 3 * C), torch.bfloat16) if variant else A.out((B, N, 3 * C), torch.float32)
        rc = L().mv_attention_bwd_long_f16(ptr(q), ptr(d16), ptr(dl), ptr(lse), ptr(gs), ptr(r["dqkv"]), variant, ptr(r["colsum"]),
                                           ptr(r["colsum_ws"]), B, N, H, scale, stream())
    else:
        d = A.inp(dout, torch.float32)
        r["delta_ws"], r["dqkv"] = A.out((B, H, N), torch.float32), A.out((B, N, 3 * C), torch.float32)
        rc = L().mv_attention_bwd_long_f32(ptr(q), ptr(out), ptr(d), ptr(lse), ptr(r["delta_ws"]), ptr(r["dqkv"]), B, N, H, scale,
                                           stream())
    assert rc == MV_OK, (name, variant, N, rc)
    A.check()
    return r


# ================================================================== the blockwise emulation (CPU)
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("dist", DISTS)
def test_blockwise_emulation_is_consistent_with_fp64(name, dist):
    """emulate(blockwise=True) at 197 keys (three full blocks and a ragged one): without roundings it reproduces fp64 autograd;
    with them it rounds, not wildly, and sits inside the bounds derived for the online form and the ceilings of the plain inputs."""
    family, dh = FAMILY[name], WIDTH[name]
    B, N, H = 2, 197, 2
    qkv, dout = random_inputs(family, dist, B, N, H, seed=3, dh=dh)
    assert torch.equal(qkv.to(OPERAND[family]).float(), qkv)
    q, k, _ = split_qkv(qkv.double(), H, dh)
    s = (q @ k.transpose(-2, -1)) * dh ** -0.5
    if dist == "peaked":
        assert float(s.abs().max()) > (60 if family == "half" else 100) and float(s.softmax(-1).amax(-1).median()) > 0.5
        first = s[..., :64].amax(-1)                         # the running maximum really moves after the first block
        assert float((s.amax(-1) > first + 1.0).double().mean()) > 0.3
    if dist == "offset":
        assert 150 < float(s.mean()) < 260 and float(s.min()) > 88.8          # exp(s) alone overflows fp32 everywhere
    want = exact_fp64(qkv, dout, H, dh)
    for a, b in zip(emulate(family, qkv, dout, H, rounded=False, dh=dh, blockwise=True), want):
        assert float((a - b).abs().max() / b.abs().max()) < 1e-11
    out, lse, dqkv = emulate(family, qkv, dout, H, dh=dh, blockwise=True)
    u = {"bf16": 2.0 ** -9, "half": 2.0 ** -12, "fp32": 2.0 ** -24}[family]
    err = slice_err(dqkv, want[2], H, dh)
    assert float(err.max()) < 1.0 and float(err.min()) > u / 64, (float(err.min()), float(err.max()))
    if family != "fp32":
        assert bool(((out - want[0]).abs() <= forward_bound(family, qkv, H, dh, blocks_of(N))).all())
        assert float(err.min()) > 2.0 ** -24 * 16
    assert bool(((lse - want[1]).abs() <= lse_bound(qkv, H, want[1], dh, blocks_of(N))).all())
    if dist == "plain":
        bars = BARS[family]
        assert rel_l2(out, want[0]) < bars["out"] and float((lse - want[1]).abs().max()) < bars["lse"]
        assert all(rel_l2(a, b) < bars["grad"] for a, b in zip(split_qkv(dqkv, H, dh), split_qkv(want[2], H, dh)))
    # the whole-head model of the same inputs: another order of the same roundings, so the same size of error
    whole = slice_err(emulate(family, qkv, dout, H, dh=dh)[2], want[2], H, dh)
    assert bool((err < 4 * whole).all()) and bool((whole < 4 * err).all())


# ================================================================== 1. routing
@gpu
@pytest.mark.parametrize("name,N", set_lengths())
def test_routing_is_exact_in_every_tiled_kernel(ops, name, N):
    """Softmax = a permutation matrix: out[i] = v[perm[i]], dv[perm[i]] = dout[i], dq = dk = 0, the column sums, the bf16 pieces
    and the q8 codes bit for bit (fp32: P is not rounded, so out / dv carry the 2 ulp of the lse -- assert_routed_forward's
    tolerance).  delta = rowsum(dO * O) is a sum of integers: exact in any order."""
    B, H = 2, 3
    family, dh = FAMILY[name], WIDTH[name]
    qkv, dout, perm, _ = routing_inputs(B, N, H, dh)
    want_out, want_dqkv, want_colsum, want_lse = routing_expected(qkv, dout, perm, H, dh)
    A = Tight()
    fw = {kind: run_fwd(A, name, qkv, B, N, H, kind) for kind in fwd_kinds(name)}
    for kind, r in fw.items():
        assert_routed_forward(family, r, want_out, want_lse, kind, (name, kind))
    if "plain" in fw:
        assert same_bits(fw["plain"]["out"], fw["lse"]["out"])
    for variant in bwd_kinds(name):
        r = run_bwd(A, name, qkv, fw["lse"], dout, B, N, H, variant)
        assert_routed_backward(ops, family, variant, r, want_dqkv, want_colsum, H, (name, variant), dh=dh)
        if family == "bf16":
            want_delta = (heads(dout, H, dh) * heads(want_out, H, dh)).sum(-1)
            assert torch.equal(r["delta_ws"].cpu(), want_delta), name
        if family == "half":
            # the per-block partials: dq and dk exact zeros; their sum over the blocks, in order, is the column sum
            C, ws = H * dh, r["colsum_ws"].cpu()
            assert bool((ws[:, :, :2 * C] == 0).all()) and torch.equal(ws.sum(1)[:, 2 * C:], want_colsum[:, 2 * C:]), variant
            rows = torch.arange(N).view(1, N, 1) // 128
            for blk in range(ws.shape[1]):                   # integers: the fp32 sums of a block are exact in any order
                part = (want_dqkv * (rows == blk)).sum(1)
                assert torch.equal(ws[:, blk, 2 * C:], part[:, 2 * C:]), (variant, blk)


# ================================================================== 2. every length against fp64
def part_errors(family, got, want, H, dh):
    """L2 relative error of dq, dk, dv.  A part that is exactly zero in exact arithmetic (dq, dk at N = 1) has no relative error:
    half and fp32 hold it against the size of the whole gradient as check_against_fp64 of tests/attention_families.py does; bf16
    -> None (the caller applies that check's absolute bound)."""
    whole, errs = float(want.norm()), []
    for a, b in zip(split_qkv(got, H, dh), split_qkv(want, H, dh)):
        den = float(b.norm())
        if family == "half":
            den = max(den, 1e-3 * whole)
        elif family == "fp32" and den <= 1e-3 * whole:
            den = whole
        errs.append(float((a - b).norm()) / den if den > 0 else None)
    return errs


@gpu
@pytest.mark.parametrize("name,N,dist", [(s, n, "plain") for s, n in set_lengths()] +
                         [(s, n, d) for d in DISTS[1:] for s, n in set_lengths(EDGE_CLASS)])
def test_every_tiled_edge_against_fp64(ops, name, N, dist):
    """Against fp64 on the same rounded inputs.  plain, at every length: the whole-tensor ceilings (BARS) and identical bits from a
    second launch.  All: the per-element forward bound (bf16, half) and the lse bound in their online forms.  peaked / offset, one
    length per edge class: each of dq, dk, dv per (image, head) within 2x the L2 error of the blockwise fp64 emulation of the kernel's
    roundings on the same inputs (fp32: the forward too, as a whole).  The fp32 family has no per-element forward bound, here as in
    tests/test_attention_short.py: without a rounding of P the bound would be the sum of the small terms alone, which the whole-head
    derivation does not claim to list completely."""
    B, H = 2, 3
    family, dh, blocks, bars = FAMILY[name], WIDTH[name], blocks_of(N), BARS[FAMILY[name]]
    qkv, dout = random_inputs(family, dist, B, N, H, seed=N, dh=dh)
    want_out, want_lse, want_dqkv = exact_fp64(qkv, dout, H, dh)
    emu_out, _, emu_dqkv = emulate(family, qkv, dout, H, dh=dh, blockwise=True)
    emu_err = slice_err(emu_dqkv, want_dqkv, H, dh)
    A = Tight()
    fw = {}
    for kind in fwd_kinds(name):
        r = fw[kind] = run_fwd(A, name, qkv, B, N, H, kind)
        if dist == "plain":
            r2 = run_fwd(A, name, qkv, B, N, H, kind)
            assert all(same_bits(r[key], r2[key]) for key in r), kind
        if kind == "q8":                                   # the codes: the quantiser applied to the plain output, bit for bit
            assert torch.equal(r["codes"].view(B * N, H * dh),
                               ops.quant_affine_i8(fw["lse"]["out"].view(B * N, H * dh), B * N, H * dh, Q8_SCALE, Q8_ZERO))
            continue
        if kind == "plain":
            assert same_bits(r["out"], fw["lse"]["out"])
            continue
        out = r["out"].double().cpu()
        e = rel_l2(out, want_out)
        print(f"fwd {name} N={N} {dist}: L2 {e:.3e}  emulation {rel_l2(emu_out, want_out):.3e}")
        if dist == "plain":
            assert e < bars["out"], e
        if family != "fp32":
            excess = ((out - want_out).abs() / forward_bound(family, qkv, H, dh, blocks)).max()
            print(f"    per-element error / bound: {float(excess):.3f}")
            assert float(excess) <= 1.0
        elif dist != "plain":
            assert e <= 2 * rel_l2(emu_out, want_out)
        d = (r["lse"].double().cpu() - want_lse).abs()
        assert bool((d <= lse_bound(qkv, H, want_lse, dh, blocks)).all())
        if dist == "plain":
            assert float(d.max()) < bars["lse"]
    plain = None
    for variant in bwd_kinds(name):
        r = run_bwd(A, name, qkv, fw["lse"], dout, B, N, H, variant)
        if dist == "plain":
            r2 = run_bwd(A, name, qkv, fw["lse"], dout, B, N, H, variant)
            assert all(same_bits(r[key], r2[key]) for key in r), variant
        if variant:                                        # the pieces of exactly the plain form's fp32 values, and its column sums
            assert torch.equal(r["dqkv"], split_of(ops, plain["dqkv"], variant)), variant
            assert same_bits(r["colsum"], plain["colsum"]) and same_bits(r["colsum_ws"], plain["colsum_ws"]), variant
            continue
        plain = r
        got = r["dqkv"].double().cpu()
        err = slice_err(got, want_dqkv, H, dh)
        names = "qkv"
        if N == 1:                                         # dq = dk = 0 exactly: only dv has a relative error
            err, names = err[2:], "v"
        ratio = (err / emu_err[-len(err):]).amax((1, 2))
        print(f"bwd {name} N={N} {dist}: worst slice L2 d{names} {[f'{float(x):.3e}' for x in err.amax((1, 2))]}  emulation "
              f"{[f'{float(x):.3e}' for x in emu_err.amax((1, 2))]}  worst ratio {[f'{float(x):.2f}' for x in ratio]}")
        if dist == "plain":
            for part, e in zip("qkv", part_errors(family, got, want_dqkv, H, dh)):
                if e is None:
                    # two fp32 sums of the same dh products in different orders (zero_gradient_bound), then one bf16 rounding of dS
                    # and one of the result: the bound of tests/attention_families.py's bf16 check
                    zb = zero_gradient_bound(qkv, dout, H, dh)[:, :, None, None] * (1 + 2.0 ** -8) ** 2
                    assert bool((split_qkv(got, H, dh)["qkv".index(part)].abs() <= zb).all()), part
                else:
                    assert e < bars["grad"], (part, e)
        else:
            assert bool((err <= 2 * emu_err).all()), [float(x) for x in ratio]
        if "colsum" in r and dist == "plain":
            cs = r["colsum"].double().cpu()
            assert rel_l2(cs, got.sum(1)) < bars["colsum_own"]
            assert rel_l2(cs, want_dqkv.sum(1)) < bars.get("colsum64", bars["grad"])
        if "colsum_ws" in r:                               # one partial per 128-row block, added in order
            ws = r["colsum_ws"]
            total = torch.zeros_like(ws[:, 0])
            for blk in range(ws.shape[1]):
                total = total + ws[:, blk]
            assert same_bits(total, r["colsum"])
            rows = (torch.arange(N).view(1, N, 1) // 128).cuda()
            for blk in range(ws.shape[1]):
                assert rel_l2(ws[:, blk].double(), (r["dqkv"].double() * (rows == blk)).sum(1)) < bars["colsum_own"], blk


# ================================================================== 3. guard zones
@gpu
@pytest.mark.parametrize("name,N", set_lengths(GUARD_N))
def test_nothing_outside_the_tensors_is_read_into_a_result_or_written(ops, name, N):
    """Every input next to NaN -- lse, delta, gscale and dout16 among them -- and every output between sentinels and prefilled with
    NaN (Guarded.check), delta_ws and colsum_ws among them: attn_delta_kernel / attn_delta_long_f32_kernel write every (image, head,
    token) of delta_ws, and with a colsum every dK / dV and dQ workgroup writes its head's columns of its own block of colsum_ws,
    so every element of both is promised.  And the bits of the same call on plain tensors."""
    B, H = 2, 3
    qkv, dout = random_inputs(FAMILY[name], "plain", B, N, H, seed=100 + N, dh=WIDTH[name])
    tight_fw = None
    for kind in fwd_kinds(name):
        t, gd = run_fwd(Tight(), name, qkv, B, N, H, kind), run_fwd(Guarded(), name, qkv, B, N, H, kind)
        assert all(same_bits(t[key], gd[key]) for key in t), kind
        tight_fw = tight_fw or t
    for variant in bwd_kinds(name):
        t = run_bwd(Tight(), name, qkv, tight_fw, dout, B, N, H, variant)
        gd = run_bwd(Guarded(), name, qkv, tight_fw, dout, B, N, H, variant)
        assert all(same_bits(t[key], gd[key]) for key in t), variant


# ================================================================== 4. independence
@gpu
@pytest.mark.parametrize("name,N", [(s, n) for s in SETS for n in INDEPENDENT_N[s]])
def test_every_image_and_head_is_computed_alone(ops, name, N):
    """A workgroup's index is (image * H + head) * blocks + block: each (image, head) slice run as a B = 1, H = 1 problem gives the
    bits of the batched run, in every output and workspace."""
    B, H = 3, 3
    family, dh = FAMILY[name], WIDTH[name]
    qkv, dout = random_inputs(family, "plain", B, N, H, seed=200 + N, dh=dh)
    A = Tight()
    fws = {kind: run_fwd(A, name, qkv, B, N, H, kind) for kind in fwd_kinds(name)}
    bws = {v: run_bwd(A, name, qkv, fws["lse"], dout, B, N, H, v) for v in bwd_kinds(name)}
    q, k, v = split_qkv(qkv, H, dh)
    do = heads(dout, H, dh)
    nb = (N + 127) // 128
    for b in range(B):
        for h in range(H):
            one = join_qkv(q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1], v[b:b + 1, h:h + 1])
            d1 = unheads(do[b:b + 1, h:h + 1]).contiguous()
            cols = slice(h * dh, (h + 1) * dh)
            fw1 = {}
            for kind, r in fws.items():
                r1 = fw1[kind] = run_fwd(A, name, one, 1, N, 1, kind)
                for key in r1:
                    full = r[key][b, h] if key == "lse" else r[key][b, :, cols]
                    assert same_bits(full.reshape(-1), r1[key].reshape(-1)), (b, h, kind, key)
            for variant, r in bws.items():
                r1 = run_bwd(A, name, one, fw1["lse"], d1, 1, N, 1, variant)
                tag = (b, h, variant)
                if variant:
                    got = r["dqkv"].view(B, N, variant, 3, H, dh)[b, :, :, :, h]
                    assert same_bits(got.contiguous(), r1["dqkv"].view(N, variant, 3, dh)), tag
                else:
                    got = r["dqkv"].view(B, N, 3, H, dh)[b, :, :, h]
                    assert same_bits(got.contiguous(), r1["dqkv"].view(N, 3, dh)), tag
                if "colsum" in r:
                    assert same_bits(r["colsum"].view(B, 3, H, dh)[b, :, h].contiguous(), r1["colsum"].view(3, dh)), tag
                if "delta_ws" in r:
                    assert same_bits(r["delta_ws"][b, h], r1["delta_ws"][0, 0]), tag
                if "colsum_ws" in r:
                    assert same_bits(r["colsum_ws"].view(B, nb, 3, H, dh)[b, :, :, h].contiguous(), r1["colsum_ws"].view(nb, 3, dh)), tag
                if "gscale" in r:
                    assert same_bits(r["gscale"][b * H + h:b * H + h + 1], r1["gscale"]), tag
                    assert same_bits(r["delta"][b, h], r1["delta"][0, 0]), tag
                    assert same_bits(r["dout16"][b, :, cols].contiguous(), r1["dout16"][0]), tag


# ================================================================== 5. zero gradient
@gpu
@pytest.mark.parametrize("name,N", set_lengths())
def test_zero_gradient_gives_exact_zeros(ops, name, N):
    B, H = 2, 2
    qkv, dout = random_inputs(FAMILY[name], "plain", B, N, H, seed=300 + N, dh=WIDTH[name])
    A = Tight()
    fw = run_fwd(A, name, qkv, B, N, H)
    for variant in bwd_kinds(name):
        r = run_bwd(A, name, qkv, fw, torch.zeros_like(dout), B, N, H, variant)
        for key in ("dqkv", "colsum", "colsum_ws", "delta_ws", "delta", "dout16"):
            assert key not in r or not r[key].any(), (variant, key)
        if "gscale" in r:
            assert bool((r["gscale"] == 1.0).all()), variant


# ================================================================== 6. API edges: nothing is launched
def api_calls(name, B, N, off=0, null_delta=False, nseg=0, null_ws=False, only=None):
    """Every entry point of the set with H = 1 on canary-filled buffers big enough for the length -> {entry: rc}, the buffers.
    off: qkv pointer offset in bytes.  only: the entries to call (a call with valid arguments would launch)."""
    H, n = 1, max(N, 1) + 1
    buf = {key: torch.full((max(B, 1) * n * 3 * 64 * 4 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
           for key in ("qkv", "out", "lse", "dout", "dqkv", "colsum", "delta", "gscale", "ws")}
    p = {key: t.data_ptr() for key, t in buf.items()}
    q, s, delta = p["qkv"] + off, stream(), None if null_delta else p["delta"]
    if name == "long":
        calls = {"fwd": lambda: L().mv_attention_fwd_long(q, p["out"], p["lse"], B, N, H, 0.125, s),
                 "bwd": lambda: L().mv_attention_bwd_long(q, p["out"], p["dout"], p["lse"], delta, p["dqkv"], p["colsum"], B, N, H,
                                                          0.125, s)}
    elif name == "long_f16":
        calls = {"fwd": lambda: L().mv_attention_fwd_long_f16(q, p["out"], p["lse"], B, N, H, 0.125, s),
                 "bwd": lambda: L().mv_attention_bwd_long_f16(q, p["dout"], delta, p["lse"], p["gscale"], p["dqkv"], nseg, p["colsum"],
                                                              None if null_ws else p["ws"], B, N, H, 0.125, s)}
    else:
        calls = {"fwd": lambda: L().mv_attention_fwd_long_f32(q, p["out"], p["lse"], B, N, H, 0.125, s),
                 "fwd_plain": lambda: L().mv_attention_fwd_long_f32(q, p["out"], None, B, N, H, 0.125, s),
                 "fwd_q8": lambda: L().mv_attention_fwd_long_f32_q8(q, p["out"], B, N, H, 0.125, Q8_SCALE, Q8_ZERO, s),
                 "bwd": lambda: L().mv_attention_bwd_long_f32(q, p["out"], p["dout"], p["lse"], delta, p["dqkv"], B, N, H, 0.125, s)}
    rcs = {key: call() for key, call in calls.items() if only is None or key in only}
    torch.cuda.synchronize()
    return rcs, buf


@gpu
@pytest.mark.parametrize("name", ["long", "long_f16", "long_f32"])
def test_api_edges_return_their_codes_and_write_nothing(ops, name):
    """The codes of include/myrtle_vision_hip.h and the MV_REQUIRE lines of the entry points (tests/test_attention_dh.py has the
    dh entry points).  Every buffer keeps its canary."""
    too_long = MV_ERR_UNSUPPORTED if name == "long_f32" else MV_ERR_SHAPE
    for (B, N, off), want in [((0, 129, 0), MV_OK), ((2, 0, 0), MV_ERR_SHAPE), ((1, 8193, 0), too_long), ((2, 129, 2), MV_ERR_ALIGN)]:
        rcs, buf = api_calls(name, B, N, off)
        assert all(rc == want for rc in rcs.values()), ((B, N, off), rcs)
        assert untouched(buf), (B, N, off)
    rcs, buf = api_calls(name, 2, 129, null_delta=True, only=("bwd",))
    assert rcs["bwd"] == MV_ERR_ALIGN and untouched(buf)
    if name == "long_f16":
        rcs, buf = api_calls(name, 2, 129, nseg=4, only=("bwd",))
        assert rcs["bwd"] == MV_ERR_UNSUPPORTED and untouched(buf)
        rcs, buf = api_calls(name, 2, 129, null_ws=True, only=("bwd",))             # a colsum without its workspace
        assert rcs["bwd"] == MV_ERR_ALIGN and untouched(buf)
