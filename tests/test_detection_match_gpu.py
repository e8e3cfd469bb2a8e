"""The device Hungarian solver (``mv_det_match``, csrc/detection.hip) against ``scipy.optimize.linear_sum_assignment``.

Where the optimum is unique the pairs must be scipy's, index for index: both are exact solvers.  Uniqueness is itself checked
with scipy (the same pairs for the matrix, its transpose and its row-and-column reversal, three different visiting orders); no
case may fail that check.  With ties only validity and the exact total cost are compared.  ``match`` and ``status`` sit in the
middle of sentinel-filled allocations (guard zones, as tests/test_attention_short.py).

Shapes: both orientations (T < Q solved transposed, T >= Q as it is), one column short of / at / one past the 64-lane wave on
either side, one and several columns per lane, and blocks that are staged in LDS and two that are not (64 KiB of costs or more
plus the solver's state exceed the 64 KiB the kernel uses, so it reads global memory): (128, 128) as it is, (700, 30) transposed."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

pytestmark = pytest.mark.gpu

from conftest import load_golden  # noqa: E402

SENTINEL = 0xA5
POISON = -(1 << 20)
SHAPES = [(100, 1), (100, 2), (100, 30), (100, 63), (100, 64), (100, 65), (100, 100), (100, 101), (100, 130), (1, 1), (1, 5),
          (7, 3), (64, 64), (65, 129), (128, 128), (300, 40), (700, 30)]
SEEDS = [0, 7, 23]


class Guarded:
    def __init__(self):
        self.items = []

    def out(self, n):
        guard = 4096
        raw = torch.full(((n * 4 + 15) // 16 * 16 + 2 * guard,), SENTINEL, dtype=torch.uint8, device="cuda")
        body = raw[guard:guard + n * 4].view(torch.int32)
        body.fill_(POISON)
        self.items.append((raw, guard, n * 4))
        return body

    def check(self):
        torch.cuda.synchronize()
        for raw, g, nb in self.items:
            assert bool((raw[:g] == SENTINEL).all()) and bool((raw[g + nb:] == SENTINEL).all()), "a guard byte changed"


def real_costs(rng, Q, T):
    """5 U - U - 2 (2 U - 1) in fp32: the range of 5 * L1 - probability - 2 * GIoU."""
    u = [rng.random((Q, T), dtype=np.float32) for _ in range(3)]
    return (np.float32(5) * u[0] - u[1] - np.float32(2) * (np.float32(2) * u[2] - np.float32(1))).astype(np.float32)


def scipy_match(c):
    """match row [Q] of scipy's assignment (-1 = unmatched)."""
    row = np.full(c.shape[0], -1, dtype=np.int64)
    if c.shape[1]:
        i, j = linear_sum_assignment(c)
        row[i] = j
    return row


def unique_optimum(c):
    a = scipy_match(c)
    i, j = linear_sum_assignment(c.T)
    b = np.full(c.shape[0], -1, dtype=np.int64)
    b[j] = i
    i, j = linear_sum_assignment(c[::-1, ::-1])
    r = np.full(c.shape[0], -1, dtype=np.int64)
    r[c.shape[0] - 1 - i] = c.shape[1] - 1 - j
    return np.array_equal(a, b) and np.array_equal(a, r)


def run(blocks, Q, max_t=None):
    """blocks: a list of fp32 [Q, T_b] arrays -> (match [B, Q] local target index or -1, status [B], raw flat match)."""
    from myrtle_vision.hip import lib
    B = len(blocks)
    sizes = [b.shape[1] for b in blocks]
    offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    flat = np.concatenate([b.reshape(-1) for b in blocks] + [np.zeros(1, np.float32)]).astype(np.float32)
    cost, toff = torch.from_numpy(flat).cuda(), torch.from_numpy(offsets).cuda()
    g = Guarded()
    match, status = g.out(B * Q), g.out(B)
    rc = lib.lib().mv_det_match(cost.data_ptr(), toff.data_ptr(), match.data_ptr(), status.data_ptr(), B, Q,
                                max(sizes) if max_t is None else max_t, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    g.check()
    m = match.cpu().numpy().reshape(B, Q).astype(np.int64)
    local = np.where(m >= 0, m - offsets[:-1, None], -1)
    return local, status.cpu().numpy(), m


def assert_valid(row, Q, T):
    hit = row[row >= 0]
    assert len(hit) == min(Q, T) and len(set(hit.tolist())) == len(hit) and (hit < T).all() and (row >= -1).all()


def total(c, row):
    q = np.nonzero(row >= 0)[0]
    return float(c[q, row[q]].astype(np.float64).sum())


# ------------------------------------------------------------------------------------------------------------ unique optimum
@pytest.mark.parametrize("seed", SEEDS)
def test_unique_optimum_gives_scipys_pairs(seed):
    """Every shape, one image per launch (so each shape sizes the kernel's LDS state itself)."""
    rng = np.random.default_rng(seed)
    dropped = 0
    for Q, T in SHAPES:
        c = real_costs(rng, Q, T)
        if not unique_optimum(c):
            dropped += 1
            continue
        local, status, _ = run([c], Q)
        assert status[0] == 0, (Q, T)
        assert np.array_equal(local[0], scipy_match(c)), (Q, T, seed)
    assert dropped == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_mixed_batch_with_an_empty_image(seed):
    rng = np.random.default_rng(1000 + seed)
    Q, sizes = 100, [30, 0, 130, 1, 100, 65, 2, 64]
    blocks = [real_costs(rng, Q, T) for T in sizes]
    assert all(unique_optimum(c) for c in blocks if c.shape[1])
    local, status, flat = run(blocks, Q)
    assert (status == 0).all()
    for b, c in enumerate(blocks):
        assert np.array_equal(local[b], scipy_match(c)), (b, sizes[b])
    # the flat index is what mv_det_assign reads: toff[b] + t
    off = np.concatenate(([0], np.cumsum(sizes)))
    assert all(((flat[b] == -1) | ((flat[b] >= off[b]) & (flat[b] < off[b + 1]))).all() for b in range(len(sizes)))
    # a max_t above the batch's largest count only sizes the state
    local2, status2, _ = run(blocks, Q, max_t=200)
    assert np.array_equal(local2, local) and (status2 == 0).all()


# ---------------------------------------------------------------------------------------------------------------------- ties
def tie_blocks():
    rng = np.random.default_rng(5)
    out = []
    for Q, T in [(100, 30), (100, 100), (64, 65), (7, 3), (100, 130), (128, 128)]:
        out.append((f"small integers {Q}x{T}", rng.integers(0, 4, (Q, T)).astype(np.float32)))
    for Q, T in [(100, 30), (5, 9), (64, 64)]:
        out.append((f"all equal {Q}x{T}", np.full((Q, T), 2.0, dtype=np.float32)))
    for Q, T in [(100, 30), (20, 64)]:
        c = np.repeat(rng.integers(0, 16, (Q, T // 2)), 2, axis=1).astype(np.float32)     # every target twice
        out.append((f"duplicated columns {Q}x{T}", c))
    return out


TIES = tie_blocks()


@pytest.mark.parametrize("c", [c for _, c in TIES], ids=[n for n, _ in TIES])
def test_ties_reach_scipys_total_and_repeat(c):
    Q, T = c.shape
    local, status, _ = run([c], Q)
    assert status[0] == 0
    assert_valid(local[0], Q, T)
    assert total(c, local[0]) == total(c, scipy_match(c))                   # integer-valued fp32: the fp64 sums are exact
    again, _, _ = run([c], Q)
    assert np.array_equal(again, local)


# ------------------------------------------------------------------------------------------------------- +inf, NaN and -inf
def test_forbidden_pairs_and_flagged_images():
    rng = np.random.default_rng(11)
    Q = 100
    feasible = real_costs(rng, Q, 30)
    feasible[rng.random((Q, 30)) < 0.3] = np.inf
    assert unique_optimum(feasible)
    wide = real_costs(rng, Q, 130)                                          # T > Q: rows are the queries
    wide[rng.random((Q, 130)) < 0.3] = np.inf
    assert unique_optimum(wide)
    blocked = real_costs(rng, Q, 30)
    blocked[:, 17] = np.inf                                                 # a target nobody may take, T <= Q
    with pytest.raises(ValueError, match="infeasible"):
        linear_sum_assignment(blocked)
    nan = real_costs(rng, Q, 65)
    nan[99, 64] = np.nan
    with pytest.raises(ValueError, match="invalid numeric"):
        linear_sum_assignment(nan)
    ninf = real_costs(rng, Q, 2)
    ninf[0, 0] = -np.inf
    with pytest.raises(ValueError, match="invalid numeric"):
        linear_sum_assignment(ninf)
    plain = real_costs(rng, Q, 64)
    assert unique_optimum(plain)
    blocks = [feasible, blocked, plain, nan, wide, ninf, np.zeros((Q, 0), np.float32), plain[:, :5].copy()]
    local, status, _ = run(blocks, Q)
    assert status.tolist() == [0, 2, 0, 1, 0, 1, 0, 0]
    for b, c in enumerate(blocks):
        if status[b]:
            assert (local[b] == -1).all()
        else:
            assert np.array_equal(local[b], scipy_match(c)), b


# ---------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks():
    from myrtle_vision.hip import lib, ops
    L, s = lib.lib(), torch.cuda.current_stream().cuda_stream
    g = Guarded()
    match, status = g.out(1100), g.out(4)
    cost, toff = torch.zeros(4096, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    a = (cost.data_ptr(), toff.data_ptr(), match.data_ptr(), status.data_ptr())
    assert L.mv_det_match(*a, 1, 100, 1025, s) == -4                        # MV_ERR_UNSUPPORTED
    assert L.mv_det_match(*a, 1, 1025, 3, s) == -4
    assert L.mv_det_match(*a, 1, 0, 3, s) == -1                             # MV_ERR_SHAPE
    assert L.mv_det_match(*a, 0, 100, 3, s) == -1
    assert L.mv_det_match(*a, 1, 100, -1, s) == -1
    g.check()
    assert bool((match == POISON).all()) and bool((status == POISON).all())  # a refused call launches nothing
    with pytest.raises(RuntimeError, match="det_match"):
        ops.det_match(cost, toff, 1, 100, 1025)
    # the limit itself runs: one image, 1024 queries, one target
    c = np.arange(1024, dtype=np.float32)[::-1].copy().reshape(1024, 1)
    local, st, _ = run([c], 1024, max_t=1024)
    assert st[0] == 0 and local[0, 1023] == 0 and (local[0, :1023] == -1).all()


# --------------------------------------------------------------------------------------------------------------- end to end
def random_batch(seed, B=4, Q=100, C=20):
    gen = torch.Generator().manual_seed(seed)
    logits, u = torch.randn(B, Q, C + 1, generator=gen), torch.rand(B, Q, 4, generator=gen)
    boxes = torch.stack((0.2 + 0.6 * u[..., 0], 0.2 + 0.6 * u[..., 1], 0.05 + 0.45 * u[..., 2], 0.05 + 0.45 * u[..., 3]), -1)
    targets = []
    for n in (0, 30, 7, 19):
        t = torch.rand(n, 4, generator=gen)
        tb = torch.stack((0.2 + 0.6 * t[:, 0], 0.2 + 0.6 * t[:, 1], 0.05 + 0.45 * t[:, 2], 0.05 + 0.45 * t[:, 3]), -1)
        targets.append({"labels": torch.randint(0, C, (n,), generator=gen).cuda(), "boxes": tb.cuda()})
    return logits.cuda(), boxes.cuda(), targets, C


def golden_batch():
    arrays, meta = load_golden("micro_det")
    targets = [{"labels": torch.from_numpy(arrays[f"tgt_labels:{b}"]).cuda(), "boxes": torch.from_numpy(arrays[f"tgt_boxes:{b}"]).cuda()}
               for b in range(meta["batch"])]
    return (torch.from_numpy(arrays["pred_logits"]).float().cuda(), torch.from_numpy(arrays["pred_boxes"]).float().cuda(), targets,
            meta["kwargs"]["num_classes"])


def make_criterion(assignment, C):
    from myrtle_vision.models.detector import SetCriterion
    from myrtle_vision.models.matcher import HungarianMatcher
    return SetCriterion(C, HungarianMatcher(assignment=assignment), {}, 0.1, ["labels", "boxes", "cardinality"]).cuda()


def criterion_run(assignment, logits, boxes, targets, C, packed=None, crit=None):
    crit = make_criterion(assignment, C) if crit is None else crit
    lg, bx = logits.clone().requires_grad_(True), boxes.clone().requires_grad_(True)
    losses = crit({"pred_logits": lg, "pred_boxes": bx}, targets, packed=packed)
    (losses["loss_ce"] + 5.0 * losses["loss_bbox"] + 2.0 * losses["loss_giou"]).backward()
    return crit, losses, lg.grad, bx.grad


@pytest.mark.parametrize("batch", ["micro_det", "random"])
def test_device_and_host_assignment_give_the_same_criterion_bits(batch):
    from myrtle_vision.models.matcher import HungarianMatcher
    logits, boxes, targets, C = golden_batch() if batch == "micro_det" else random_batch(3)
    host_crit, host, hdl, hdb = criterion_run("host", logits, boxes, targets, C)
    dev_crit, dev, ddl, ddb = criterion_run("device", logits, boxes, targets, C)
    assert host_crit.match_status is None
    assert dev_crit.match_status.is_cuda and dev_crit.match_status.dtype == torch.int32
    assert dev_crit.match_status.cpu().tolist() == [0] * logits.shape[0]
    assert list(dev) == list(host) and len(dev) == 5
    for k in host:
        assert torch.equal(dev[k].detach().cpu().view(torch.int32), host[k].detach().cpu().view(torch.int32)), k
    assert torch.equal(ddl, hdl) and torch.equal(ddb, hdb)
    out = {"pred_logits": logits, "pred_boxes": boxes}
    want, got = HungarianMatcher()(out, targets), HungarianMatcher(assignment="device")(out, targets)
    assert len(want) == len(got)
    for (i, j), (wi, wj) in zip(got, want):
        assert i.dtype == j.dtype == torch.int64 and not i.is_cuda and not j.is_cuda
        assert torch.equal(i, wi) and torch.equal(j, wj)


def test_device_matcher_raises_scipys_message_for_a_bad_label():
    """A label outside the classes makes mv_det_cost write NaN: scipy's ValueError in host mode, the same one in device mode."""
    from myrtle_vision.models.matcher import HungarianMatcher
    logits, boxes, targets, C = random_batch(4)
    targets[2]["labels"][3] = C + 5
    out = {"pred_logits": logits, "pred_boxes": boxes}
    with pytest.raises(ValueError) as host:
        HungarianMatcher()(out, targets)
    with pytest.raises(ValueError) as dev:
        HungarianMatcher(assignment="device")(out, targets)
    assert str(dev.value) == str(host.value)


# ------------------------------------------------------------------------------------------------------- no host round trip
def test_device_criterion_and_backward_never_wait_for_the_host():
    """torch's sync debug mode raises at every synchronising call.  The control is the host-mode criterion on the same inputs,
    which copies the cost blocks to the host and must raise; the device-mode criterion and its backward must not."""
    from myrtle_vision.models.matcher import PackedTargets
    logits, boxes, targets, C = random_batch(5)
    packed = PackedTargets(targets, logits.device)
    host_crit, dev_crit = make_criterion("host", C), make_criterion("device", C)      # the weights reach the device here
    criterion_run("device", logits, boxes, targets, C, packed=packed, crit=dev_crit)  # first use: library load, allocations
    torch.cuda.synchronize()
    prior = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            criterion_run("host", logits, boxes, targets, C, packed=packed, crit=host_crit)
        crit, losses, dl, db = criterion_run("device", logits, boxes, targets, C, packed=packed, crit=dev_crit)
    finally:
        torch.cuda.set_sync_debug_mode(prior)
    torch.cuda.synchronize()
    assert crit.match_status.cpu().tolist() == [0, 0, 0, 0]
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(db).all()) and bool(torch.isfinite(losses["loss_ce"]))
