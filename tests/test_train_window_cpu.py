"""The gradient-accumulation window of the training loops (``engine.AccumWindow``) on fakes, without a GPU: the exact sequence of
``zero_grad`` / ``backward`` / ``finish`` / ``clip_accumulated`` / ``step`` and the reducer's ``enabled`` flag at every backward.  The
expected sequences are literals, written down from the loop the window replaced."""
import pytest


class _Optimizer:
    def __init__(self, log):
        self.log = log

    def zero_grad(self):
        self.log.append("zero_grad")

    def step(self):
        self.log.append("step")

    def clip_accumulated(self):
        self.log.append("clip_accumulated")


class _Reducer:
    def __init__(self, log, world):
        self.log, self.world, self.enabled = log, world, None

    def finish(self):
        self.log.append("finish")


class _Loss:
    def __init__(self, log, reducer):
        self.log, self.reducer = log, reducer

    def backward(self):
        self.log.append(("backward", self.reducer.enabled))


def _window(n_batch_accum, clip_every, world):
    from myrtle_vision.engine import AccumWindow
    log = []
    reducer = _Reducer(log, world)
    return AccumWindow(_Optimizer(log), reducer, n_batch_accum, clip_every), _Loss(log, reducer), log


def test_one_micro_batch_per_step():
    window, loss, log = _window(1, False, world=1)
    assert [window.backward(loss) for _ in range(2)] == [True, True]
    assert log == ["zero_grad", ("backward", False), "finish", "step"] * 2


def test_three_micro_batches_exchange_only_the_last():
    window, loss, log = _window(3, False, world=2)
    assert [window.backward(loss) for _ in range(3)] == [False, False, True]
    assert log == ["zero_grad", ("backward", False), ("backward", False), ("backward", True), "finish", "step"]


def test_clipping_exchanges_and_clips_after_every_micro_batch_but_the_last():
    window, loss, log = _window(3, True, world=2)
    assert [window.backward(loss) for _ in range(3)] == [False, False, True]
    assert log == ["zero_grad", ("backward", True), "finish", "clip_accumulated", ("backward", True), "finish", "clip_accumulated",
                   ("backward", True), "finish", "step"]


def test_clipping_in_one_process_never_enables_the_reducer_and_still_finishes():
    window, loss, log = _window(2, True, world=1)
    assert [window.backward(loss) for _ in range(4)] == [False, True, False, True]
    assert log == ["zero_grad", ("backward", False), "finish", "clip_accumulated", ("backward", False), "finish", "step"] * 2


@pytest.mark.parametrize("world", [1, 2])
def test_a_window_opened_by_one_epoch_is_completed_by_the_next(world):
    window, loss, log = _window(2, False, world=world)
    at_start, stepped = [], []
    for epoch in (3, 2):                                     # five micro-batches: the third opens a window the fourth closes
        for _ in range(epoch):
            at_start.append(window.at_start)
            stepped.append(window.backward(loss))
    assert at_start == [True, False, True, False, True]      # before batches 1, 3 and 5 only
    assert stepped == [False, True, False, True, False]      # after batches 2 and 4
    first, last = ("backward", False), ("backward", world > 1)
    assert log == ["zero_grad", first, last, "finish", "step", "zero_grad", first, last, "finish", "step", "zero_grad", first]
    assert not window.at_start
