"""mv_gemm_tn_bf16_group: several weight gradients over one contraction range in one equal-split launch.

Every buffer the library writes (each C, the workspace) sits inside a larger allocation filled with a canary bit pattern; after
each call the canary must still be everywhere the result is not: before and after every C, between the rows of a C whose ldc is
wider than N, in the workspace past the slabs, and past the workspace end.  References are float64 products of the same
bf16-rounded inputs, bar 3e-6 of the largest element as in tests/test_hip_ops.py::test_gemm_tn_every_variant (what is left is
fp32 accumulation order)."""
import ctypes

import pytest
import torch

CANARY = 0x7FC0DEAD          # a quiet NaN nobody computes
GUARD = 1024                 # floats on each side


def _lib():
    from myrtle_vision.hip.lib import lib
    return lib()


def _check(rc, what):
    from myrtle_vision.hip.lib import check
    check(rc, what)


def _item_type():
    from myrtle_vision.hip.ops import _TnItem
    return _TnItem


def g(seed):
    return torch.Generator().manual_seed(seed)


def relerr(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


class Guarded:
    """``n`` fp32 elements at a 16-byte aligned address with GUARD canary floats on both sides."""

    def __init__(self, n):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")
        assert self.raw.data_ptr() % 16 == 0

    @property
    def body(self):
        return self.raw[GUARD:GUARD + self.n].view(torch.float32)

    def ptr(self):
        return self.body.data_ptr()

    def guards_intact(self):
        return bool((self.raw[:GUARD] == CANARY).all()) and bool((self.raw[GUARD + self.n:] == CANARY).all())

    def canary_at(self, mask_or_slice):
        return bool((self.raw[GUARD:GUARD + self.n][mask_or_slice] == CANARY).all())


def plan256(tiles, Kc):
    """tn_plan256's rule (csrc/gemm_bf16.hip) on a tile count: (splits, stages per split)."""
    nk = Kc // 32
    s = max(1, min(256 // tiles, -(-nk // 16)))
    steps = -(-nk // s)
    return -(-nk // steps), steps


def tiles_of(M, N):
    return -(-M // 256) * -(-N // 256)


_inputs = {}


def operands(Kc, M, N, lda, ldb, seed):
    """bf16 A [Kc, lda], B [Kc, ldb] (pad columns zero) on the device and the float64 product A[:, :M]^T B[:, :N]; made once."""
    key = (Kc, M, N, lda, ldb, seed)
    if key not in _inputs:
        a = torch.zeros(Kc, lda)
        b = torch.zeros(Kc, ldb)
        a[:, :M] = torch.randn(Kc, M, generator=g(seed))
        b[:, :N] = torch.randn(Kc, N, generator=g(seed + 100))
        a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
        want = a[:, :M].double().t() @ b[:, :N].double()
        _inputs[key] = (a.cuda(), b.cuda(), want)
    return _inputs[key]


def run_group(shapes, Kc, force):
    """``shapes``: list of (M, N, lda, ldb, ldc).  Runs the group under TN force code ``force`` inside guard zones, checks the
    canaries and returns the list of C [M, N] tensors (copies) and the references."""
    lib = _lib()
    Item = _item_type()
    items = (Item * len(shapes))()
    cs, wants, keep = [], [], []
    for i, (M, N, lda, ldb, ldc) in enumerate(shapes):
        a, b, want = operands(Kc, M, N, lda, ldb, 10 + i)
        c = Guarded(M * ldc)
        it = items[i]
        it.A, it.lda, it.B, it.ldb, it.C, it.ldc, it.M, it.N = a.data_ptr(), lda, b.data_ptr(), ldb, c.ptr(), ldc, M, N
        cs.append(c)
        wants.append(want)
        keep.append((a, b))
    addr = ctypes.addressof(items)
    nbytes = lib.mv_gemm_tn_group_workspace_bytes(addr, len(shapes), Kc)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Guarded(nbytes // 4)
    _check(lib.mv_gemm_force_variant(0, force), "force_variant")
    try:
        _check(lib.mv_gemm_tn_bf16_group(addr, len(shapes), Kc, ws.ptr(), nbytes, torch.cuda.current_stream().cuda_stream),
               "gemm_tn_bf16_group")
        torch.cuda.synchronize()
    finally:
        _check(lib.mv_gemm_force_variant(0, 0), "force_variant")
    assert ws.guards_intact(), "write outside the workspace"
    if force == 256 and Kc % 32 == 0:       # grouped: the slabs are splits x (items' [M][N] blocks, each rounded up to 4 floats) and nothing else
        splits, _ = plan256(sum(tiles_of(M, N) for M, N, *_ in shapes), Kc)
        used = splits * sum((M * N + 3) // 4 * 4 for M, N, *_ in shapes) if splits > 1 else 0
        assert used <= ws.n
        assert ws.canary_at(slice(used, None)), "write in the workspace past the slabs"
        # ... and the grouped kernel really ran: every element of every item's block of every slab was written, the floats that
        # round a block up to a multiple of 4 were not (items run one by one lay their slabs out differently and fail this)
        written = ws.raw[GUARD:GUARD + used] != CANARY
        expect = torch.zeros(used, dtype=torch.bool, device="cuda")
        if splits > 1:
            stride, off = used // splits, 0
            for M, N, *_ in shapes:
                for s in range(splits):
                    expect[s * stride + off:s * stride + off + M * N] = True
                off += (M * N + 3) // 4 * 4
        assert torch.equal(written, expect), "the slabs are not the grouped launch's"
    outs = []
    for (M, N, lda, ldb, ldc), c in zip(shapes, cs):
        assert c.guards_intact(), "write outside C"
        body = c.body.view(M, ldc)
        if ldc > N:
            pad = torch.zeros(M, ldc, dtype=torch.bool, device="cuda")
            pad[:, N:] = True
            assert c.canary_at(pad.view(-1)), "write between the rows of C"
        out = body[:, :N].clone()
        assert not bool((out.view(torch.int32) == CANARY).any()), "an element of C was never written"
        outs.append(out)
    return outs, wants


def run_single(M, N, lda, ldb, ldc, Kc, seed):
    """mv_gemm_tn_bf16 with the 256-tile kernel forced: what the parent computes for this product."""
    lib = _lib()
    a, b, _ = operands(Kc, M, N, lda, ldb, seed)
    c = torch.empty(M, ldc, dtype=torch.float32, device="cuda")
    nbytes = lib.mv_gemm_tn_workspace_bytes(M, N, Kc)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _check(lib.mv_gemm_force_variant(0, 256), "force_variant")
    try:
        _check(lib.mv_gemm_tn_bf16(a.data_ptr(), lda, b.data_ptr(), ldb, c.data_ptr(), ldc, M, N, Kc, 0, None, ws.data_ptr(), nbytes,
                                   torch.cuda.current_stream().cuda_stream), "gemm_tn_bf16")
        torch.cuda.synchronize()
    finally:
        _check(lib.mv_gemm_force_variant(0, 0), "force_variant")
    return c[:, :N].clone()


PAIR = [(256, 256, 256, 256, 256), (768, 256, 768, 256, 256)]
RAGGED = [(264, 136, 264, 136, 136), (72, 520, 72, 520, 520)]
# the ragged pair made awkward: an odd N (block of 264 x 135 floats is no multiple of 4: the next item's slab offset is
# rounded up), lda / ldb wider than the item, ldc wider than N (the reduce's scalar form, canary between the rows)
ODD = [(264, 135, 272, 136, 140), (72, 520, 72, 528, 520), (8, 8, 8, 8, 8)]
GROUPS = {"pair-1024": (PAIR, 1024), "pair-4096": (PAIR, 4096), "ragged-2048": (RAGGED, 2048), "odd-2048": (ODD, 2048),
          "one-4096": (PAIR[1:], 4096), "one-ragged-2048": (RAGGED[:1], 2048), "one-split-512": (PAIR, 512)}


def test_plan_of_the_listed_groups():
    """What the cases exercise: 4 tiles -> 2 splits at Kc 1024; more splits at 4096; the one-split group writes C itself."""
    assert plan256(sum(tiles_of(M, N) for M, N, *_ in PAIR), 1024) == (2, 16)
    assert plan256(sum(tiles_of(M, N) for M, N, *_ in PAIR), 4096) == (8, 16)
    assert plan256(sum(tiles_of(M, N) for M, N, *_ in RAGGED), 2048) == (4, 16)
    assert plan256(sum(tiles_of(M, N) for M, N, *_ in PAIR), 512)[0] == 1


def test_force_code_and_workspace_size_need_no_gpu():
    lib = _lib()
    try:
        for ok in (0, 128, 256, 1000, 1128, 1256):
            assert lib.mv_gemm_force_variant(0, ok) == 0
        for bad in (1, 1001, 2256, 2000, -1):
            assert lib.mv_gemm_force_variant(0, bad) != 0
    finally:
        assert lib.mv_gemm_force_variant(0, 0) == 0
    Item = _item_type()
    items = (Item * 2)()
    for it, (M, N) in zip(items, ((768, 768), (2304, 768))):
        it.M, it.N, it.lda, it.ldb, it.ldc = M, N, M, N, N
    addr = ctypes.addressof(items)
    nbytes = lib.mv_gemm_tn_group_workspace_bytes(addr, 2, 50432)
    # ViT-B at batch 256: 36 tiles -> 7 splits of both blocks; never less than either product wants alone (the fallback)
    assert plan256(36, 50432)[0] == 7
    assert nbytes >= 7 * (768 * 768 + 2304 * 768) * 4
    assert nbytes >= max(lib.mv_gemm_tn_workspace_bytes(768, 768, 50432), lib.mv_gemm_tn_workspace_bytes(2304, 768, 50432))
    assert lib.mv_gemm_tn_group_workspace_bytes(addr, 0, 50432) == 0 and lib.mv_gemm_tn_group_workspace_bytes(addr, 5, 50432) == 0
    assert lib.mv_gemm_tn_bf16_group(addr, 5, 50432, None, 0, None) != 0          # rejected before anything is launched


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GROUPS))
def test_group_matches_float64_is_deterministic_and_stays_in_bounds(name):
    shapes, Kc = GROUPS[name]
    outs, wants = run_group(shapes, Kc, 256)
    again, _ = run_group(shapes, Kc, 256)
    for out, out2, want in zip(outs, again, wants):
        assert relerr(out, want) < 3e-6
        assert torch.equal(out, out2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one-4096", "one-ragged-2048"])
def test_one_item_group_is_mv_gemm_tn_bf16_bit_for_bit(name):
    shapes, Kc = GROUPS[name]
    (out,), _ = run_group(shapes, Kc, 256)
    assert torch.equal(out, run_single(*shapes[0], Kc, 10))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pair-1024", "pair-4096", "ragged-2048", "odd-2048"])
def test_pairing_switched_off_reproduces_the_single_products(name):
    shapes, Kc = GROUPS[name]
    outs, wants = run_group(shapes, Kc, 1256)
    for i, (shape, out, want) in enumerate(zip(shapes, outs, wants)):
        assert torch.equal(out, run_single(*shape, Kc, 10 + i))
        assert relerr(out, want) < 3e-6


@pytest.mark.gpu
def test_ragged_contraction_runs_the_items_one_by_one():
    """Kc = 1000 is no multiple of 32: no grouped launch, each item as mv_gemm_tn_bf16 runs it (ring on 992 rows + the rest)."""
    outs, wants = run_group(RAGGED, 1000, 1256)
    grouped, _ = run_group(RAGGED, 1000, 256)
    for i, (shape, a, b, want) in enumerate(zip(RAGGED, outs, grouped, wants)):
        assert torch.equal(a, b) and torch.equal(a, run_single(*shape, 1000, 10 + i))
        assert relerr(a, want) < 3e-6


def test_only_linear_dw_pair_may_defer_a_product():
    """``linear_dw(_pair=...)`` returns gradients that are not computed yet; nothing but ``linear_dw_pair`` can ask for that."""
    from myrtle_vision.hip import ops
    t = torch.zeros(32, 8, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="linear_dw_pair"):
        ops.linear_dw(t, t, 32, 8, 8, _pair=[])
