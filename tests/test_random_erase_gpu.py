"""Random Erasing on the device: the two kernels of csrc/random_erase.hip, the ``RandomErasing`` class, the captured training step and
the engine's loop.

References: the draw is pinned bit for bit to the numpy restatement (tests/random_erase_ref.py over oracle/dropout_oracle.py); the
fill's exact parts (what is written where, and what is left alone) to index arithmetic; the fill's values to the fp64 Box-Muller of
the same exact uniforms.  The bar for the values is 8 x the error of the SAME fp32 formula, sqrt(-2 ln u1) * {cos, sin}(2 pi u2),
evaluated with torch's fp32 ops on the device against fp64, measured over this test's own words -- not derived from the kernel
under test (the rule of profiles/detection_parity.txt; the figures are in profiles/random_erase_parity.txt)."""
import copy
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import random_erase_ref as R
from random_erase_ref import Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, STEP = (5 << 40) + 12345, (1 << 32) - 1            # both halves of the key in use; step + 1 carries into the counter's high word


@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def _state(seed, step):
    return torch.tensor([seed, step], dtype=torch.int64).cuda()


# ================================================================== 1. the draw
DRAWS = {
    "zero-extent": ((5, 7, 9), dict(probability=1.0, min_count=2, max_count=3, min_area=0.002, max_area=0.05)),
    "more-samples-than-threads": ((257, 32, 48), dict(probability=0.5)),
    "defaults": ((64, 224, 224), dict()),
    "failing-attempts": ((6, 16, 16), dict(probability=1.0, min_area=0.9, max_area=0.9, min_aspect=0.1)),
}


@pytest.mark.parametrize("case", list(DRAWS))
def test_draw_is_the_restatement_and_advances_the_step(ops, case):
    from myrtle_vision.hip import lib
    (B, H, W), kw = DRAWS[case]
    full = dict(probability=0.25, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, min_count=1, max_count=None)
    full.update(kw)
    max_aspect = 1 / full["min_aspect"] if full["max_aspect"] is None else full["max_aspect"]
    max_count = full["min_count"] if full["max_count"] is None else full["max_count"]
    args = dict(thr=int(full["probability"] * 2 ** 32), min_area=full["min_area"], max_area=full["max_area"],
                log_ratio=(math.log(full["min_aspect"]), math.log(max_aspect)), min_count=full["min_count"], max_count=max_count)
    want = [R.draw(B, H, W, SEED, STEP + s, **kw) for s in (0, 1)]
    excluded = sum(len(R.near_half(w[1])) for w in want)
    assert excluded == 0                                   # the seeds were chosen so: every attempt is compared
    state = _state(SEED, STEP)
    boxes0, used0 = ops.random_erase_draw(state, B, H, W, **args)
    # the second call through the C ABI itself, into arrays that sit between guard zones
    G = Guarded(torch)
    boxes1 = G.new((B, max_count, 4), torch.int32, torch.full((B, max_count, 4), -1, dtype=torch.int32))
    used1 = G.new((2,), torch.int64, torch.full((2,), -1, dtype=torch.int64))
    area_ratio = (ctypes.c_double * 4)(args["min_area"], args["max_area"], *args["log_ratio"])      # a host array
    rc = lib.lib().mv_random_erase_draw(state.data_ptr(), boxes1.data_ptr(), used1.data_ptr(), B, H, W, args["thr"],
                                        ctypes.addressof(area_ratio), args["min_count"], max_count,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    G.check()
    assert boxes0.shape == (B, max_count, 4) and boxes0.dtype == torch.int32 and boxes0.data_ptr() != boxes1.data_ptr()
    assert np.array_equal(boxes0.cpu().numpy(), want[0][0])
    assert np.array_equal(boxes1.cpu().numpy(), want[1][0])
    assert used0.tolist() == [SEED, STEP] and used1.tolist() == [SEED, STEP + 1]
    assert state.tolist() == [SEED, STEP + 2]
    assert not np.array_equal(want[0][0], want[1][0])
    b = want[0][0]
    if case == "zero-extent":                              # accepted boxes that erase nothing: one extent rounded to zero
        assert ((b[..., 2] == 0) ^ (b[..., 3] == 0)).any()
    if case == "failing-attempts":                         # ten failures leave the slot empty; some attempts do succeed
        assert 0 < int((b[:, 0, 2] > 0).sum()) < B and len(want[0][1]) > 5 * B


# ================================================================== 2. the fill, exact parts
def _tables(H, W):
    """int32 [4, 3, 4]: a box at the origin, one ending in the last row and column, one of zero extent; two overlapping boxes and
    an empty slot; a sample with no box; three boxes that overlap pairwise and all together."""
    return torch.tensor([
        [[0, 0, 2, 3], [H - 3, W - 4, 3, 4], [1, 1, 0, 5]],
        [[1, 1, 4, 5], [3, 3, 4, 4], [0, 0, 0, 0]],
        [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]],
        [[2, 0, 3, W], [0, 2, H, 3], [1, 1, 3, 3]],
    ], dtype=torch.int32)


def _big_shape(ops):
    """A shape whose boxes need more than one pass of the fill's grid: more box rows (Ch * h) than bands * waves row workers, with
    the number of bands at its cap."""
    Ch = 3
    H = ops.RANDOM_ERASE_ROWS_PER_BLOCK * ops.RANDOM_ERASE_MAX_BANDS // Ch + 60
    assert Ch * H > ops.RANDOM_ERASE_ROWS_PER_BLOCK * ops.RANDOM_ERASE_MAX_BANDS              # the band count is capped ...
    assert Ch * (H - 1) > 4 * ops.RANDOM_ERASE_MAX_BANDS * ops.RANDOM_ERASE_WAVES             # ... and a box goes round > 4 times
    return Ch, H, 9


def _planted(shape, dtype, seed):
    """A random batch that also holds -0.0, a NaN with a payload, and denormals of both signs, spread over the whole tensor."""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)
    flat = bits(x).view(-1)                                # a view: x is contiguous, so the patterns land in x itself
    assert flat.data_ptr() == x.data_ptr()
    pats = [0x80000000, 0x7FC01234, 0x00000001, 0x807FFFFF] if dtype == torch.float32 else [0x8000, 0x7FC5, 0x0001, 0x807F]
    wrap = (1 << 32) if dtype == torch.float32 else (1 << 16)
    for j, p in enumerate(pats):
        flat[j * 3::7 * len(pats)] = p - wrap if p >= wrap // 2 else p
    assert bool(x.isnan().any()) and bool((x == 0).any())
    return x


FILL_SHAPES = [(1, 8, 9), (3, 8, 48), (3, 8, 9), (1, 8, 48), "big"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", FILL_SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_fill_writes_the_boxes_and_nothing_else(ops, shape, dtype):
    Ch, H, W = _big_shape(ops) if shape == "big" else shape
    table = _tables(H, W)
    if shape == "big":
        table[0, 0] = torch.tensor([0, 0, H - 1, W - 1])                 # Ch * (H - 1) rows: several passes of the row workers
        table[3, 1] = torch.tensor([1, 2, H - 1, 3])
    B = table.shape[0]
    x = _planted((B, Ch, H, W), dtype, 70 + Ch + W)
    owner = torch.from_numpy(R.winners(table.numpy(), H, W))              # [B, H, W]
    inside = (owner >= 0)[:, None].expand(B, Ch, H, W)
    assert int((owner[0] >= 0).sum()) > 0 and int((owner[2] >= 0).sum()) == 0 and bool((owner[1] == 0).any()) and bool((owner[3] == 2).any())
    got = {}
    for mode in ("const", "rand", "pixel", "pixel-again"):
        G = Guarded(torch)
        xd = G.new((B, Ch, H, W), dtype, x)
        bd = G.new(tuple(table.shape), torch.int32, table)
        used = G.new((2,), torch.int64, torch.tensor([SEED, STEP], dtype=torch.int64))
        out = ops.random_erase_apply(xd, bd, used, mode.split("-")[0])
        torch.cuda.synchronize()
        assert out.data_ptr() == xd.data_ptr()                           # in place
        G.check()
        assert torch.equal(bd.cpu(), table) and used.tolist() == [SEED, STEP]
        got[mode] = bits(xd.cpu())
        assert torch.equal(got[mode][~inside], bits(x)[~inside]), mode   # outside every box: the input's bits, whatever they were
    assert bool((got["const"][inside] == 0).all())                       # +0.0, exactly, on the union of the boxes
    assert torch.equal(got["pixel"], got["pixel-again"])                 # a function of (used, element index) alone
    assert not torch.equal(got["pixel"][inside], got["const"][inside])
    colours = {}
    for b in range(B):
        for k in range(table.shape[1]):
            for c in range(Ch):
                vals = got["rand"][b, c][owner[b] == k]
                if vals.numel():
                    assert bool((vals == vals[0]).all()), (b, k, c)      # one bit pattern per (box, channel), the LATER box's in an overlap
                    colours[(b, k, c)] = int(vals[0])
    # and another one for every other (sample, box, channel): all distinct in fp32; bf16 has 2^16 patterns, so two may coincide
    assert len(colours) > 4 and len(set(colours.values())) >= (len(colours) if dtype == torch.float32 else len(colours) // 2 + 1)


# ================================================================== 3. the fill, values
def _bf16_bounds(v64, bar):
    lo, hi = R.bf16_round((v64 - bar).astype(np.float32)), R.bf16_round((v64 + bar).astype(np.float32))
    return lo.astype(np.float64), hi.astype(np.float64)


def test_fill_values_against_fp64(ops):
    """``pixel`` and ``rand`` against the fp64 restatement.  The bar: 8 x the largest error of torch's fp32 evaluation of the same
    Box-Muller formula on the device, over the words this test uses (measured on an MI355X: profiles/random_erase_parity.txt).
    bf16 is the fp32 value rounded to nearest even: bit-equal to the fp32 run's values rounded by torch, and inside the fp64 value's
    own rounding interval [bf16(v - bar), bf16(v + bar)]; the elements where that interval holds two bf16 values are counted."""
    B, Ch, H, W = 4, 3, 32, 48
    boxes, _, _ = R.draw(B, H, W, SEED, STEP, probability=1.0, min_count=2, max_count=2, min_area=0.1, max_area=0.3)
    shape = (B, Ch, H, W)
    own_p, ref_p = R.fill64(shape, boxes, "pixel", SEED, STEP)
    own_r, ref_r = R.fill64(shape, boxes, "rand", SEED, STEP)
    inside = np.broadcast_to((own_p >= 0)[:, None], shape)
    assert 2000 < int(inside.sum()) < inside.size
    # the bar, from torch's fp32 ops on the device over the same words
    a_p, b_p, s_p = R.pixel_words(np.arange(inside.size, dtype=np.uint64).reshape(shape)[inside], SEED, STEP)
    trip = [R.colour_words(b, k, c, Ch, SEED, STEP) for b in range(B) for k in range(2) for c in range(Ch)]
    a = np.concatenate([a_p, np.array([t[0] for t in trip], dtype=np.uint64)])
    b = np.concatenate([b_p, np.array([t[1] for t in trip], dtype=np.uint64)])
    s = np.concatenate([s_p, np.zeros(len(trip), dtype=bool)])
    ad, bd, sd = (torch.from_numpy(v.astype(np.int64)).cuda() for v in (a, b, s))
    u1, u2 = ((ad >> 9).float() + 0.5) * 2.0 ** -23, ((bd >> 9).float() + 0.5) * 2.0 ** -23
    assert u1.dtype == torch.float32
    t = (2.0 * math.pi) * u2
    z32 = torch.sqrt(-2.0 * torch.log(u1)) * torch.where(sd.bool(), torch.sin(t), torch.cos(t))
    torch_err = float(np.abs(z32.double().cpu().numpy() - R.normal64(a, b, s)).max())
    bar = 8.0 * torch_err
    print(f"torch fp32 Box-Muller against fp64 over {a.size} word pairs: max |error| {torch_err:.3e}; bar = 8 x = {bar:.3e}")
    assert 1e-8 < torch_err < 1e-5                                       # an fp32 evaluation: a few ulp of values up to ~5

    table = torch.from_numpy(boxes)
    outs = {}
    for mode, ref in (("pixel", ref_p), ("rand", ref_r)):
        for dtype in (torch.float32, torch.bfloat16):
            G = Guarded(torch)
            xd = G.new(shape, dtype, torch.ones(shape, dtype=dtype))
            ops.random_erase_apply(xd, table.cuda(), _state(SEED, STEP), mode)
            torch.cuda.synchronize()
            G.check()
            outs[mode, dtype] = xd.cpu()
            assert bool((outs[mode, dtype].float().numpy()[~inside] == 1.0).all())
        v64 = ref[inside]
        got32 = outs[mode, torch.float32].numpy()[inside].astype(np.float64)
        err = float(np.abs(got32 - v64).max())
        print(f"{mode} fp32: max |kernel - fp64| {err:.3e} over {v64.size} elements (bar {bar:.3e}); largest |value| {np.abs(v64).max():.3f}")
        assert err <= bar, (mode, err, bar)
        # bf16: the kernel's fp32 value, rounded once to nearest even
        assert same_bits(outs[mode, torch.bfloat16], outs[mode, torch.float32].to(torch.bfloat16)), mode
        got16 = outs[mode, torch.bfloat16].float().numpy()[inside].astype(np.float64)
        lo, hi = _bf16_bounds(v64, bar)
        straddle = int((lo != hi).sum())
        off = int((got16 != R.bf16_round(v64.astype(np.float32)).astype(np.float64)).sum())
        print(f"{mode} bf16: {straddle} of {v64.size} elements have a rounding boundary inside v +- bar; {off} differ from bf16(fp64 value)")
        assert bool(((lo <= got16) & (got16 <= hi)).all()), mode
        assert off <= straddle
    # pixel noise is standard normal; rand colours differ between boxes and channels
    z = outs["pixel", torch.float32].numpy()[inside].astype(np.float64)
    assert abs(z.mean()) <= 4 / math.sqrt(z.size) and abs(z.var() - 1) <= 4 * math.sqrt(2 / z.size)


# ================================================================== 4. the class
def test_class_erases_the_restated_boxes(ops, monkeypatch):
    from myrtle_vision.utils.random_erasing import RandomErasing
    B, Ch, H, W = 7, 3, 40, 56
    e = RandomErasing(probability=1.0, mode="const", min_count=1, max_count=3)
    e.seed(SEED, STEP)
    x = torch.ones(B, Ch, H, W).cuda()
    y = e(x)
    torch.cuda.synchronize()
    assert y.data_ptr() == x.data_ptr() and e.state.tolist() == [SEED, STEP + 1]
    boxes, _, _ = R.draw(B, H, W, SEED, STEP, probability=1.0, min_count=1, max_count=3)
    assert np.array_equal(e.last_boxes.cpu().numpy(), boxes)
    erased = torch.from_numpy(R.winners(boxes, H, W) >= 0)
    assert bool(erased.any()) and not bool(erased.all())
    want = torch.where(erased[:, None].expand(B, Ch, H, W), 0.0, 1.0)
    assert same_bits(y, want)
    # a non-contiguous batch: a contiguous, erased result (the stream goes on: step + 1)
    nc = torch.ones(B, H, W, Ch).cuda().permute(0, 3, 1, 2)
    assert not nc.is_contiguous()
    z = e(nc)
    torch.cuda.synchronize()
    boxes2, _, _ = R.draw(B, H, W, SEED, STEP + 1, probability=1.0, min_count=1, max_count=3)
    assert z.is_contiguous() and np.array_equal(e.last_boxes.cpu().numpy(), boxes2)
    erased2 = torch.from_numpy(R.winners(boxes2, H, W) >= 0)
    assert same_bits(z, torch.where(erased2[:, None].expand(B, Ch, H, W), 0.0, 1.0))
    # bf16, the default mode: erased elements are noise, the others untouched
    p = RandomErasing(probability=1.0)
    p.seed(SEED, STEP)
    xb = torch.ones(B, Ch, H, W, dtype=torch.bfloat16).cuda()
    p(xb)
    own = torch.from_numpy(R.winners(p.last_boxes.cpu().numpy(), H, W) >= 0)[:, None].expand(B, Ch, H, W)
    assert bool((xb.cpu()[~own] == 1).all()) and float((xb.cpu()[own] != 1).float().mean()) > 0.95

    # probability 0: nothing is drawn, nothing is launched
    def boom(*a, **kw):
        raise AssertionError("a random-erase op ran with the probability at 0")
    monkeypatch.setattr(ops, "random_erase_draw", boom)
    monkeypatch.setattr(ops, "random_erase_apply", boom)
    off = RandomErasing(probability=0.0)
    assert off(x) is x and off.last_boxes is None and off.state is None


# ================================================================== 5. captured step
def _micro(**kw):
    from myrtle_vision.models.vit import ViT
    base = dict(decoder="classification", image_size=224, patch_size=16, num_classes=10, dim=128, depth=3, heads=2, mlp_dim=256)
    base.update(kw)
    return ViT(**base)


def _batch(B=6, seed=17):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 224, 224, generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()


def test_captured_step_erases_anew_on_every_replay(ops):
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.utils.graph import GraphedTrainStep
    from myrtle_vision.utils.optim import AdamW, ParamArena
    from myrtle_vision.utils.random_erasing import RandomErasing
    from myrtle_vision.utils.utils import seed_everything
    ERASE_SEED = 977
    batches = [_batch(6, 60 + i) for i in range(4)]

    def build():
        seed_everything(23)
        vit = _micro(precision="bf16", q_format="FP32").cuda().train()
        eraser = RandomErasing(probability=0.6)
        eraser.seed(ERASE_SEED)
        opt = AdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-3, weight_decay=0.05)
        return vit, opt, eraser, (lambda m, x, y: cross_entropy(m(eraser(x)), y))

    # eager: the step erases its input buffer in place, and the graphed step's warm-up runs three times on ONE buffer
    vit_e, opt_e, eraser_e, loss_e = build()
    buf, losses_e = batches[0][0].clone(), []
    for i in [0, 0, 0, 1, 2, 3]:
        if i:
            buf.copy_(batches[i][0])
        opt_e.zero_grad()
        loss = loss_e(vit_e, buf, batches[i][1])
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss.detach()))
    vit_g, opt_g, eraser_g, loss_g = build()
    graphed = GraphedTrainStep(vit_g, opt_g, loss_g, *batches[0], warmup=3)
    assert eraser_g.state.tolist() == [ERASE_SEED, 3]                          # three warm-up steps; the capture itself ran nothing
    losses_g, tables = [], []
    for k, i in enumerate((1, 2, 3)):
        losses_g.append(float(graphed(*batches[i])))
        torch.cuda.synchronize()
        assert eraser_g.state.tolist() == [ERASE_SEED, 4 + k]
        tables.append(eraser_g.last_boxes.cpu().numpy().copy())
        assert np.array_equal(tables[-1], R.draw(6, 224, 224, ERASE_SEED, 3 + k, probability=0.6)[0])
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])
    assert all(t.any() for t in tables)
    assert losses_g == losses_e[3:]
    assert torch.equal(opt_g.arena.flat_param, opt_e.arena.flat_param)


# ================================================================== 6. the engine's loop
def _engine_config(tmp_path):
    """ViT-Tiny at depth 2 on a synthetic RESISC-45 directory with 16 training images: two iterations at batch 8."""
    from myrtle_vision.datasets.synthetic import make_resisc45
    cfg = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_tiny.json")))
    data = json.load(open(os.path.join(ROOT, "classification", "data_configs", "data_config.json")))
    data["dataset_path"] = make_resisc45(str(tmp_path / "NWPU-RESISC45"), classes=12, per_class=2)
    dpath = str(tmp_path / "data_config.json")
    json.dump(data, open(dpath, "w"))
    cfg["data_config_path"] = dpath
    cfg["train_config"].update(output_directory=str(tmp_path / "ckpt"), epochs=1, local_batch_size=8, global_batch_size=8,
                               iters_per_checkpoint=1000, iters_per_val=1000, distributed=False, pretrained_backbone=None,
                               drop_last_batch=False,          # the 2 validation images make one (partial) validation batch
                               reprob=1.0, remode="const", recount=2)
    cfg["vit_config"]["depth"] = 2
    return cfg


def test_engine_erases_each_training_batch_and_no_validation_batch(tmp_path, capsys, monkeypatch):
    from myrtle_vision.engine import train_worker
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.random_erasing import RandomErasing
    events = []
    erase_call, vit_forward = RandomErasing.__call__, ViT.forward

    def recording_erase(self, imgs):
        before = imgs.clone()
        out = erase_call(self, imgs)
        events.append(("erase", before, out.clone(), self.last_boxes.cpu().numpy().copy(), (self.mode, self.min_count, self.max_count)))
        return out

    def recording_forward(self, x, *a, **kw):
        events.append(("train" if self.training else "val", x.clone()))
        return vit_forward(self, x, *a, **kw)

    monkeypatch.setattr(RandomErasing, "__call__", recording_erase)
    monkeypatch.setattr(ViT, "forward", recording_forward)
    iters = train_worker(0, 1, copy.deepcopy(_engine_config(tmp_path)), "classification")
    out = capsys.readouterr().out
    losses = [float(l.split("loss=")[1].split()[0]) for l in out.splitlines() if l.startswith("Iteration")]
    assert iters == 2 and len(losses) == 2 and all(math.isfinite(l) and abs(l) < 50 for l in losses) and "nan" not in out.lower()
    kinds = [e[0] for e in events]
    assert kinds.count("erase") == 2 and kinds.count("train") == 2 and kinds.count("val") >= 1       # once per micro-batch, never in validation
    for i, e in enumerate(events):
        if e[0] != "erase":
            continue
        _, before, after, boxes, conf = e
        assert conf == ("const", 2, 2)
        assert events[i + 1][0] == "train" and torch.equal(events[i + 1][1], after)                  # the model is handed the erased batch
        erased = torch.from_numpy(R.winners(boxes, after.shape[-2], after.shape[-1]) >= 0)[:, None].expand(after.shape).cuda()
        assert bool(erased.any()) and bool((after[erased] == 0).all()) and torch.equal(after[~erased], before[~erased])
        assert not torch.equal(before, after)
    for e in events:
        if e[0] == "val":                                  # no validation batch carries a zeroed rectangle of an erase
            assert float((e[1] == 0).float().mean()) < 0.01
