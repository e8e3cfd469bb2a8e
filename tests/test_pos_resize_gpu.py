"""Positional-embedding resize on the GPU (mv_pos_resize_fwd / _bwd, reference vit.py:292-302): the two ops alone against torch's
fp64 CPU bicubic, the autograd function inside the model, and what the model keeps between grids.

Kernel tolerances follow the project's convention (tests/test_detection_gpu.py): 8 x the error of torch's own fp32 CPU evaluation
of the same quantity against fp64, computed here for the same input, with a floor of a few fp32 roundings so that a case torch
happens to compute exactly cannot make the bound zero.  Outputs sit in the middle of larger allocations filled with a sentinel
(guard zones, as tests/test_attention_short.py).

MV_POS_RESIZE_PARITY=<file>: every reference error and kernel error is appended there (profiles/pos_resize_parity.txt is to be
such a run); all of them are printed."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                   # unit roundoff of fp32
SENTINEL = 0xA5
SRC = (14, 14)
GRIDS = [(14, 14), (1, 1), (3, 5), (15, 14), (16, 16), (20, 33), (40, 66), (7, 28)]
DIMS = [4, 64, 192]
CASES = [(SRC, g, D) for g in GRIDS for D in DIMS] + [((3, 4), g, 64) for g in [(3, 4), (1, 1), (7, 9), (2, 3)]]
IDS = [f"{s[0]}x{s[1]}-{g[0]}x{g[1]}-D{D}" for s, g, D in CASES]


def record(tag, ref_err, err, bound):
    line = f"{tag}: torch fp32 vs fp64 {ref_err:.3e}, kernel vs fp64 {err:.3e}, bound {bound:.3e}"
    print(line)
    path = os.environ.get("MV_POS_RESIZE_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------------------ references
def torch_resize(pos, src, grid):
    """pos [1 + sh*sw, D] (any float dtype, CPU) -> [1 + gh*gw, D] exactly as reference vit.py:292-302 does it."""
    (sh, sw), (gh, gw) = src, grid
    D = pos.shape[1]
    g = pos[1:].t().reshape(1, D, sh, sw)
    g = TF.interpolate(g, size=grid, mode="bicubic", align_corners=False)
    return torch.cat((pos[:1], g.reshape(D, gh * gw).t()), dim=0)


_R = {}


def weight_matrix(src, grid, dtype=torch.float64):
    """R [gh*gw, sh*sw] of torch's CPU bicubic in ``dtype``: the resize of the one-hot grids.  Computed once per case."""
    key = (src, grid, dtype)
    if key not in _R:
        n = src[0] * src[1]
        eye = torch.eye(n, dtype=dtype).reshape(1, n, *src)
        r = TF.interpolate(eye, size=grid, mode="bicubic", align_corners=False)
        _R[key] = r.reshape(n, grid[0] * grid[1]).t().contiguous()
    return _R[key]


def torch_resize_vjp(g, src, grid):
    """g [1 + gh*gw, D] (CPU) -> d/dpos of <resize(pos), g> by autograd through F.interpolate, in g's dtype."""
    pos = torch.zeros(1 + src[0] * src[1], g.shape[1], dtype=g.dtype, requires_grad=True)
    torch_resize(pos, src, grid).backward(g)
    return pos.grad


def inputs(src, grid, D):
    gen = torch.Generator().manual_seed(1000 * grid[0] + 10 * grid[1] + D + src[0])
    x = torch.randn(1 + src[0] * src[1], D, generator=gen)
    g = torch.randn(1 + grid[0] * grid[1], D, generator=gen)
    return x, g


# ------------------------------------------------------------------------------------------------------------ guard zones
class Guarded:
    """Output tensors in the middle of sentinel-filled allocations, bodies prefilled with NaN."""

    def __init__(self):
        self.items = []

    def out(self, shape, fill=float("nan")):
        n = int(np.prod(shape))
        guard = 4096
        raw = torch.full((n * 4 + 2 * guard,), SENTINEL, dtype=torch.uint8, device="cuda")
        body = raw[guard:guard + n * 4].view(torch.float32).view(shape)
        assert body.data_ptr() % 16 == 0
        if isinstance(fill, torch.Tensor):
            body.copy_(fill)
        else:
            body.fill_(fill)
        self.items.append((raw, guard, n * 4))
        return body

    def check(self):
        torch.cuda.synchronize()
        for raw, guard, nb in self.items:
            assert bool((raw[:guard] == SENTINEL).all()) and bool((raw[guard + nb:] == SENTINEL).all()), "a guard byte changed"


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops
    return ops


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("src,grid,D", CASES, ids=IDS)
def test_forward_matches_torch_bicubic(ops, src, grid, D):
    x, _ = inputs(src, grid, D)
    G = Guarded()
    out = ops.pos_resize_fwd(x.cuda(), *grid, *src, out=G.out((1 + grid[0] * grid[1], D)))
    G.check()
    out = out.cpu()
    assert bool(torch.isfinite(out).all())                                   # every element written
    assert torch.equal(bits(out[0]), bits(x[0]))                             # the cls row passes through, bit for bit
    if grid == src:
        assert torch.equal(bits(out), bits(x))                               # identity: bit for bit
    want = torch_resize(x.double(), src, grid)
    ref_err = float((torch_resize(x, src, grid).double() - want).abs().max())
    err = float((out.double() - want).abs().max())
    bound = max(8 * ref_err, 4 * U * float(x.abs().max()))
    record(f"fwd {src}->{grid} D={D}", ref_err, err, bound)
    assert err <= bound


@pytest.mark.parametrize("src,grid", [(SRC, g) for g in GRIDS] + [((3, 4), (7, 9))], ids=lambda v: f"{v[0]}x{v[1]}")
def test_forward_of_one_hot_grids_is_torchs_weight_matrix(ops, src, grid):
    """Channel q holds the one-hot grid of source cell q, so out[1 + p, q] = R[p, q]: a transposed or shifted tap that random data
    could hide inside its tolerance shows as a wrong weight here."""
    n = src[0] * src[1]
    assert n % 4 == 0
    x = torch.cat((torch.zeros(1, n), torch.eye(n)), dim=0)
    G = Guarded()
    out = ops.pos_resize_fwd(x.cuda(), *grid, *src, out=G.out((1 + grid[0] * grid[1], n)))
    G.check()
    got = out.cpu()[1:].double()
    want = weight_matrix(src, grid)
    ref_err = float((weight_matrix(src, grid, torch.float32).double() - want).abs().max())
    err = float((got - want).abs().max())
    bound = max(8 * ref_err, 4 * U * 1.0)                                   # max |x| = 1
    record(f"one-hot {src}->{grid}", ref_err, err, bound)
    assert err <= bound
    assert bool((out.cpu()[0] == 0).all())


# ------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("src,grid,D", CASES, ids=IDS)
def test_backward_matches_torch_autograd(ops, src, grid, D):
    _, g = inputs(src, grid, D)
    G = Guarded()
    dpos = ops.pos_resize_bwd(g.cuda(), *grid, sh=src[0], sw=src[1], out=G.out((1 + src[0] * src[1], D)))   # over a NaN fill
    again = ops.pos_resize_bwd(g.cuda(), *grid, sh=src[0], sw=src[1], out=G.out((1 + src[0] * src[1], D), fill=7.0))
    G.check()
    dpos, again = dpos.cpu(), again.cpu()
    assert bool(torch.isfinite(dpos).all())                                  # accumulate = 0 overwrites every cell
    assert torch.equal(bits(dpos), bits(again))                              # two runs, the same bits, whatever was there before
    assert torch.equal(bits(dpos[0]), bits(g[0]))                            # the cls row passes through
    want = torch_resize_vjp(g.double(), src, grid)
    ref_err = float((torch_resize_vjp(g, src, grid).double() - want).abs().max())
    # Floor, per cell: the cell is sum_p R[p, q] * dout[p]; every product and every partial sum is a number of size at most
    # S[q] = sum_p |R[p, q]| * |dout[p]| and is rounded to 2^-24 of it, so four such roundings (a product, two additions, the store)
    # are the least any fp32 evaluation can be asked for: 4 * 2^-24 * S[q], with |R| from torch's fp64 weights.
    S = torch.cat((g[:1].double().abs(), weight_matrix(src, grid).abs().t() @ g[1:].double().abs()), dim=0)
    err = (dpos.double() - want).abs()
    bound = torch.clamp(4 * U * S, min=8 * ref_err)
    record(f"bwd {src}->{grid} D={D}", ref_err, float(err.max()), float(bound.min()))
    assert bool((err <= bound).all()), float((err - bound).max())
    untouched = torch.cat((torch.zeros(1, dtype=torch.bool), weight_matrix(src, grid).abs().sum(dim=0) == 0))
    assert bool((dpos[untouched] == 0).all())                                # cells no target row reads get exactly zero


@pytest.mark.parametrize("src,grid,D", CASES, ids=IDS)
def test_backward_is_the_adjoint_of_forward(ops, src, grid, D):
    """<fwd(x), g> against <x, bwd(g)> on the device's own fp32 results, both inner products accumulated in fp64."""
    x, g = inputs(src, grid, D)
    y = ops.pos_resize_fwd(x.cuda(), *grid, *src).cpu().double()
    d = ops.pos_resize_bwd(g.cuda(), *grid, sh=src[0], sw=src[1]).cpu().double()
    lhs, rhs = float((y * g.double()).sum()), float((x.double() * d).sum())
    # Both kernels evaluate sum_pq g[p] R[p, q] x[q] with the SAME fp32 per-axis weights, so only their roundings differ, each 2^-24
    # relative to a term of S = sum_pq |g[p]| |R[p, q]| |x[q]| (first order).  Forward, along the path of one term: the product with
    # the x weight, at most 3 additions across the row, the product with the y weight, at most 3 additions across rows, = 8.
    # Backward: the taps clamped onto one cell are added per axis (at most 3 + 3 additions), the two weights multiplied (1), the
    # product with dout (1), then the cell's terms are added by 8 thread rows of ceil(nnz / 8) terms each and the 8 partial sums one
    # after the other (7); terms with a zero weight add exactly.  The cls row is a copy on both sides.
    R = weight_matrix(src, grid)
    nnz = int((R != 0).sum(dim=0).max())
    roundings = 8 + (6 + 1 + 1 + (nnz + 7) // 8 + 7)
    S = float(((R.abs() @ x[1:].double().abs()) * g[1:].double().abs()).sum())
    bound = 1.01 * roundings * U * S
    print(f"adjoint {src}->{grid} D={D}: |lhs - rhs| {abs(lhs - rhs):.3e}, bound {bound:.3e} ({roundings} roundings)")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("src,grid,D", [(SRC, (3, 5), 64), (SRC, (20, 33), 192), (SRC, (14, 14), 4), ((3, 4), (7, 9), 64)],
                         ids=["down", "up", "identity", "src3x4"])
def test_backward_accumulates_into_a_prefilled_gradient(ops, src, grid, D):
    _, g = inputs(src, grid, D)
    pre = torch.randn(1 + src[0] * src[1], D, generator=torch.Generator().manual_seed(5))
    G = Guarded()
    fresh = ops.pos_resize_bwd(g.cuda(), *grid, sh=src[0], sw=src[1], out=G.out(pre.shape))
    acc = ops.pos_resize_bwd(g.cuda(), *grid, sh=src[0], sw=src[1], out=G.out(pre.shape, fill=pre), accumulate=True)
    G.check()
    fresh, acc = fresh.cpu(), acc.cpu()
    want = pre.double() + fresh.double()                                     # exact in fp64: two fp32 numbers
    assert bool(((acc.double() - want).abs() <= U * want.abs()).all())       # one fp32 rounding of the sum
    untouched = torch.cat((torch.zeros(1, dtype=torch.bool), weight_matrix(src, grid).abs().sum(dim=0) == 0))
    assert bool(untouched.any()) == (grid == (3, 5))                         # downscaling leaves source cells unread
    assert torch.equal(bits(acc[untouched]), bits(pre[untouched]))           # no contribution: exactly the pre-fill


def test_bad_arguments_are_refused_before_launch(ops):
    x = torch.zeros(197, 8, device="cuda")
    with pytest.raises(RuntimeError, match="pos_resize_fwd"):
        ops.pos_resize_fwd(x, 1025, 3)
    with pytest.raises(RuntimeError, match="pos_resize_bwd"):
        ops.pos_resize_bwd(torch.zeros(16, 6, device="cuda"), 3, 5)
    with pytest.raises(RuntimeError, match="pos_resize_fwd"):
        ops.pos_resize_fwd(x.view(-1)[1:197 * 4 + 1].view(197, 4), 3, 5)        # 4 bytes off 16-byte alignment
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ model level
def micro_vit(dim=64, **kw):
    from myrtle_vision.models.vit import ViT
    torch.manual_seed(3)
    return ViT(decoder="detection", image_size=224, patch_size=16, num_classes=20, dim=dim, depth=2, heads=1, dim_head=dim,
               mlp_dim=2 * dim, num_det_tokens=10, q_format="FP32", precision="fp32", **kw).cuda()


@pytest.mark.parametrize("shape", [(3, 48, 80), (2, 256, 256)], ids=["3x48x80", "2x256x256"])
def test_model_gradient_of_the_positional_embedding(shape):
    """pos_embedding.grad of the micro detector against the fp64 composition R^T sum_b dx, dx = the gradient that reaches the
    embedding output (taken with a hook); the gradient is written in place in its arena slot."""
    from myrtle_vision.utils.optim import ParamArena
    B, H, W = shape
    grid = (H // 16, W // 16)
    vit = micro_vit()
    arena = ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names())
    arena.flat_grad.fill_(float("nan"))
    arena.zero_grad()
    seen = {}

    def watch(module, args):                                                 # args[0]: the embedding output [B, T, D]
        args[0].register_hook(lambda gr: seen.__setitem__("dx", gr.detach().clone()))

    handle = vit.dropout.register_forward_pre_hook(watch)
    gen = torch.Generator().manual_seed(8)
    img = torch.randn(B, 3, H, W, generator=gen).cuda()
    out = vit(img)
    wl, wb = torch.randn(out["pred_logits"].shape, generator=gen).cuda(), torch.randn(out["pred_boxes"].shape, generator=gen).cuda()
    ((out["pred_logits"] * wl).sum() + (out["pred_boxes"] * wb).sum()).backward()
    torch.cuda.synchronize()
    handle.remove()
    assert not vit.__dict__.get("_pos_resize_cache")                         # the matrix fallback was not used
    dx = seen["dx"].float().cpu()                                            # [B, 1 + gh*gw, D]
    assert dx.shape == (B, 1 + grid[0] * grid[1], 64)
    want = torch_resize_vjp(dx.double().sum(dim=0), SRC, grid)
    ref_err = float((torch_resize_vjp(dx.sum(dim=0), SRC, grid).double() - want).abs().max())
    got = vit.pos_embedding.grad
    assert got is not None and got.shape == vit.pos_embedding.shape
    err = float((got[0].cpu().double() - want).abs().max())
    record(f"model grad {shape} {grid}", ref_err, err, 8 * ref_err)
    assert err <= 8 * ref_err
    j = list(arena.names).index("pos_embedding")
    assert got.data_ptr() == arena.slot(j).data_ptr()                        # written in place, not copied in by sync_grads()


def test_new_grids_leave_nothing_behind():
    """Forwards at eight distinct grids in a row: the fallback's cache stays empty, and resizing at eight more grids allocates
    nothing that outlives the results."""
    vit = micro_vit().eval()
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for gh, gw in [(3, 5), (4, 4), (5, 3), (6, 7), (7, 5), (8, 8), (9, 4), (3, 4)]:
            out = vit(torch.randn(1, 3, 16 * gh, 16 * gw, generator=gen).cuda())
            assert out["pred_logits"].shape == (1, 10, 21) and bool(torch.isfinite(out["pred_logits"]).all())
        assert not vit.__dict__.get("_pos_resize_cache")
        del out
        vit._pos_embedding(2, 2)                                             # first launch of the kernel's code object
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for gh, gw in [(20, 33), (21, 33), (22, 40), (25, 38), (30, 45), (40, 66), (33, 20), (66, 40)]:
            r = vit._pos_embedding(gh, gw)
            assert r.shape == (1, 1 + gh * gw, 64)
            del r
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    assert not vit.__dict__.get("_pos_resize_cache")


def test_unsupported_width_runs_through_the_bounded_fallback():
    """D = 6 is not a multiple of 4: the matrix path computes it, to the bound tests/test_detection_data_gpu.py holds that path
    to, and its cache keeps the stated number of most recently used grids."""
    from myrtle_vision.hip import ops
    vit = micro_vit(dim=6).eval()
    keep = vit._POS_RESIZE_CACHE_GRIDS
    assert keep == 4 and not ops.pos_resize_supported(6, 3, 5)
    p = vit.pos_embedding.detach().cpu()
    grids = [(3, 5), (4, 4), (5, 3), (6, 7), (7, 5), (8, 8), (16, 16)]
    assert len(grids) > keep
    with torch.no_grad():
        for grid in grids:
            got = vit._pos_embedding(*grid).cpu()
            want = torch_resize(p[0], SRC, grid).unsqueeze(0)
            # fp32 dot products of 196 terms: |error| <= 196 * 2^-24 * sum|w| * max|x|, sum|w| < 2 for the 2-D bicubic kernel
            bound = 196 * U * 2.0 * float(p.abs().max())
            assert got.shape == want.shape and float((got - want).abs().max()) <= bound
            assert len(vit._pos_resize_cache) <= keep
        assert [k[:2] for k in vit._pos_resize_cache] == grids[-keep:]
        vit._pos_embedding(*grids[-keep])                                    # a hit moves the grid to the recent end
        vit._pos_embedding(2, 2)
        assert [k[:2] for k in vit._pos_resize_cache] == [(8, 8), (16, 16), (6, 7), (2, 2)]
