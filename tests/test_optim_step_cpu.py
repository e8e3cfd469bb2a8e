"""The frame of ``AdamW.step`` / ``TableAdamW.step`` without a GPU: the three ``ops`` entry points are replaced by recorders, and the
recorded order and keyword arguments are held to literals -- count first, then the optional clip reduction, then the launches
(two for the plain class, decay group first; one for the table class), then ``bump_versions``."""
import pytest
import torch

GRAD_SCALE, MAX_NORM = 0.5, 0.25


def _vit():
    from myrtle_vision.models.vit import ViT
    return ViT(image_size=224, patch_size=16, dim=64, depth=2, heads=1, mlp_dim=128, decoder="classification", num_classes=5)


def _optimizer(table):
    from myrtle_vision.utils.optim import AdamW, ParamArena, TableAdamW
    vit = _vit()
    arena = ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names())
    kw = dict(lr=1e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.05)
    if table:
        return TableAdamW(arena, layer_decay=0.75, no_weight_decay=["pos_embedding"], ema_decay=0.9, **kw)
    return AdamW(arena, **kw)


@pytest.fixture
def calls(monkeypatch):
    """[(entry point, positional arguments, keyword arguments)] in call order; ``clip_out`` is what the clip reduction returns."""
    from myrtle_vision.hip import ops

    class Calls(list):
        clip_out = torch.tensor([3.0, 0.125])
    rec = Calls()

    def recorder(name, result=None):
        def f(*args, **kw):
            rec.append((name, args, kw))
            return result
        return f
    monkeypatch.setattr(ops, "adamw_step", recorder("adamw_step"))
    monkeypatch.setattr(ops, "adamw_table_step", recorder("adamw_table_step"))
    monkeypatch.setattr(ops, "grad_norm_clip", recorder("grad_norm_clip", rec.clip_out))
    return rec


def _same(view, base, lo=0, hi=None):
    """``view`` is ``base[lo:hi]``: same storage, same start, same length."""
    hi = base.numel() if hi is None else hi
    return view.data_ptr() == base[lo:hi].data_ptr() and view.numel() == hi - lo


def _step(opt, calls, clip):
    opt.grad_scale = GRAD_SCALE
    opt.max_grad_norm = MAX_NORM if clip else None
    opt.step_count = 6
    versions = [p._version for p in opt.arena.params]
    opt.step()
    assert opt.step_count == 7                                                  # and 7 is the ``step`` every launch received
    assert all(p._version > v for p, v in zip(opt.arena.params, versions))      # bump_versions ran after the launches
    a = opt.arena
    if clip:
        name, args, kw = calls.pop(0)                                           # the reduction comes before any launch
        assert name == "grad_norm_clip" and kw == {}
        assert _same(args[0], a.flat_grad) and args[1:] == (MAX_NORM, GRAD_SCALE)
        assert opt.last_grad_norm is calls.clip_out
    else:
        assert opt.last_grad_norm is None
    for _, _, kw in calls:
        coef = kw.pop("clip_coef")
        if clip:                                                                # the [1:2] view of what the reduction returned
            assert coef.shape == (1,) and coef.data_ptr() == calls.clip_out[1:2].data_ptr()
        else:
            assert coef is None
    return calls


@pytest.mark.parametrize("clip", [False, True])
def test_plain_step_is_two_launches_decay_group_first(calls, clip):
    opt = _optimizer(table=False)
    opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = 2e-3, 3e-3           # each launch carries ITS group's rate
    a, nd = opt.arena, opt.arena.n_decay
    assert 0 < nd < a.total
    launches = _step(opt, calls, clip)
    assert [name for name, _, _ in launches] == ["adamw_step", "adamw_step"]
    for (_, args, kw), (lo, hi), lr, wd in zip(launches, [(0, nd), (nd, a.total)], [2e-3, 3e-3], [0.05, 0.0]):
        assert len(args) == 4
        for view, base in zip(args, (a.flat_param, a.flat_grad, opt.exp_avg, opt.exp_avg_sq)):
            assert _same(view, base, lo, hi)
        assert kw == dict(lr=lr, beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=wd, step=7, grad_scale=GRAD_SCALE, hyper=None)


@pytest.mark.parametrize("clip", [False, True])
def test_table_step_is_one_launch_over_the_arena(calls, clip):
    opt = _optimizer(table=True)
    a = opt.arena
    launches = _step(opt, calls, clip)
    assert [name for name, _, _ in launches] == ["adamw_table_step"]
    _, args, kw = launches[0]
    assert len(args) == 7
    for got, want in zip(args[:4], (a.flat_param, a.flat_grad, opt.exp_avg, opt.exp_avg_sq)):
        assert got is want                                                      # the whole arena, not a slice
    assert args[4] is opt.items and args[5] is opt.seg_lr_scale and args[6] is opt.seg_wd
    ema = kw.pop("ema")
    assert ema is opt.ema and ema is not None
    assert kw == dict(lr=1e-3, beta1=0.8, beta2=0.95, eps=1e-6, step=7, grad_scale=GRAD_SCALE, hyper=None, ema_decay=0.9)


def test_table_step_without_an_ema_passes_none_and_zero(calls):
    from myrtle_vision.utils.optim import ParamArena, TableAdamW
    vit = _vit()
    opt = TableAdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-3, layer_decay=0.75)
    opt.step()
    (name, _, kw), = calls
    assert name == "adamw_table_step" and kw["ema"] is None and kw["ema_decay"] == 0.0 and kw["step"] == 1
