"""Host side of the device Hungarian matcher (no GPU): the function that turns ``mv_det_match``'s result into the reference's
index lists, its two error messages, and the ``assignment`` argument.

The expected lists are scipy's own: for every hand-written ``match`` row a cost matrix is built whose unique optimum is that row
(0 on the chosen pairs, 1 + a distinct positive amount everywhere else), and ``linear_sum_assignment`` on it is the reference."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment


def cost_with_optimum(row, T):
    """[Q, T] fp64 matrix whose only minimum-cost assignment pairs query q with target row[q] (>= 0)."""
    Q = len(row)
    c = 1.0 + np.arange(Q * T, dtype=np.float64).reshape(Q, T) / (Q * T + 1)
    for q, t in enumerate(row):
        if t >= 0:
            c[q, t] = 0.0
    return c


# per image: (T_b, local match row of length Q)
Q = 6
IMAGES = {
    "no targets": (0, [-1, -1, -1, -1, -1, -1]),
    "fewer targets": (3, [-1, 2, -1, 0, -1, 1]),
    "one target": (1, [-1, -1, -1, -1, 0, -1]),
    "as many targets": (6, [5, 3, 0, 1, 4, 2]),
    "more targets": (9, [7, 0, 8, 3, 1, 5]),            # every query matched
}
BATCHES = [["no targets"], ["more targets"], ["fewer targets", "no targets", "more targets", "one target", "as many targets"]]


@pytest.mark.parametrize("names", BATCHES, ids=lambda n: "+".join(n))
def test_index_lists_equal_scipy(names):
    from myrtle_vision.models.matcher import indices_from_match
    sizes = [IMAGES[n][0] for n in names]
    offsets = np.concatenate(([0], np.cumsum(sizes))).tolist()
    match = np.concatenate([[offsets[b] + t if t >= 0 else -1 for t in IMAGES[n][1]] for b, n in enumerate(names)]).astype(np.int32)
    got = indices_from_match(match, np.zeros(len(names), dtype=np.int32), Q, offsets)
    assert len(got) == len(names)
    for (i, j), n in zip(got, names):
        T, row = IMAGES[n]
        assert i.dtype == j.dtype == torch.int64 and not i.is_cuda and not j.is_cuda
        assert len(i) == len(j) == min(Q, T)
        wi, wj = linear_sum_assignment(cost_with_optimum(row, T)) if T else ([], [])
        assert np.array_equal(i.numpy(), np.asarray(wi, dtype=np.int64)), (n, i, wi)
        assert np.array_equal(j.numpy(), np.asarray(wj, dtype=np.int64)), (n, j, wj)


def test_status_raises_scipys_messages():
    from myrtle_vision.models.matcher import indices_from_match, raise_for_status
    match = np.full(2 * Q, -1, dtype=np.int32)
    nan = np.ones((3, 3))
    nan[1, 1] = np.nan
    with pytest.raises(ValueError) as invalid:
        linear_sum_assignment(nan)
    inf = np.ones((3, 3))
    inf[:, 1] = np.inf
    with pytest.raises(ValueError) as infeasible:
        linear_sum_assignment(inf)
    for status, want in ((1, invalid), (2, infeasible)):
        with pytest.raises(ValueError) as got:
            indices_from_match(match, np.array([0, status], dtype=np.int32), Q, [0, 2, 4])
        assert str(got.value) == str(want.value)
        with pytest.raises(ValueError) as got:
            raise_for_status(torch.tensor([status, 0], dtype=torch.int32).numpy())
        assert str(got.value) == str(want.value)
    raise_for_status(np.zeros(4, dtype=np.int32))


def test_assignment_argument():
    from myrtle_vision.models.matcher import HungarianMatcher
    assert HungarianMatcher().assignment == "host"
    assert HungarianMatcher(assignment="host").assignment == "host"
    assert HungarianMatcher(1, 5, 2, assignment="device").assignment == "device"
    with pytest.raises(ValueError, match="bogus"):
        HungarianMatcher(assignment="bogus")


def test_oversize_batch_takes_the_host_path_with_one_warning():
    import warnings

    from myrtle_vision.hip import ops
    from myrtle_vision.models import matcher as M

    class Sizes:
        def __init__(self, sizes):
            self.sizes = sizes
    m = M.HungarianMatcher(assignment="device")
    small, wide = {"pred_logits": torch.zeros(2, 100, 5)}, {"pred_logits": torch.zeros(1, ops.DET_MATCH_MAX + 1, 5)}
    M._warned_host_fallback = False
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert m.on_device(small, Sizes([0, ops.DET_MATCH_MAX]))
        assert not m.on_device(small, Sizes([3, ops.DET_MATCH_MAX + 1]))
        assert not m.on_device(wide, Sizes([3]))
        assert not M.HungarianMatcher().on_device(small, Sizes([3, 4]))
    assert len(seen) == 1 and "host" in str(seen[0].message)
