"""The three launch statements of csrc/ that no other test reaches (profiles/launch_all.txt, section 3), each at the smallest shape with
more than one workgroup and a ragged edge, against the reference its neighbours in test_hip_ops.py use."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops as _ops
    return _ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def bf(t):
    return t.to(torch.bfloat16)


def test_weight_prep_with_odd_leading_dimensions(ops):
    """weight_prep_kernel (32 x 32 tiles, one element per lane): taken when a leading dimension is odd, which ops.prepared_weight
    (pad8) never asks for.  Same contract as the 64-tile form: w as bf16 and its transpose, pad columns zero."""
    from myrtle_vision.hip.lib import check, lib
    R, C, ldw, ldt = 37, 135, 137, 39
    w = torch.randn(R, C, generator=g(2))
    wd = w.cuda()
    wb = torch.full((R, ldw), 7.0, dtype=torch.bfloat16, device="cuda")
    wt = torch.full((C, ldt), 7.0, dtype=torch.bfloat16, device="cuda")
    check(lib().mv_weight_prep(wd.data_ptr(), wb.data_ptr(), ldw, wt.data_ptr(), ldt, R, C, ops._s()), "weight_prep")
    torch.cuda.synchronize()
    assert torch.equal(wb[:, :C].cpu(), bf(w)) and (wb[:, C:] == 0).all()
    assert torch.equal(wt[:, :R].cpu(), bf(w.t())) and (wt[:, R:] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_quant_affine_codes_with_a_column_count_that_is_no_multiple_of_four(ops, dtype):
    """quant_affine_codes_kernel (one element per lane): cols % 4 != 0.  The codes are the integers q - z of
    torch.fake_quantize_per_tensor_affine, exactly; the pad columns are zero; the GELU pre-op agrees with gelu + quantiser up to one
    code where the 1.5e-7-accurate erf moves a value across a rounding boundary (about one element in 10^5: at most one of these 675)."""
    M, K = 5, 135
    x = (torch.randn(M, K, generator=g(1)) * 2 + 0.3).to(dtype)
    xf = x.float()
    s_x = float((xf.max() - min(xf.min(), 0)) / 255.0)
    z_x = int(min(max(round(-float(min(xf.min(), 0)) / s_x), 0), 255))
    xq = torch.fake_quantize_per_tensor_affine(xf, s_x, z_x, 0, 255)
    xc = ops.quant_affine_codes(x.cuda(), M, K, s_x, z_x, 0, 255)
    assert xc.shape == (M, 136) and xc.dtype == torch.bfloat16
    assert torch.equal(xc[:, :K].float().cpu(), torch.round(xq / s_x)) and (xc[:, K:] == 0).all()
    fused = ops.quant_affine_codes(x.cuda(), M, K, s_x, z_x, 0, 255, pre_gelu=True).float()
    plain = ops.quant_affine_codes(ops.gelu_fwd(xf.cuda()), M, K, s_x, z_x, 0, 255).float()
    assert float((fused - plain).abs().max()) <= 1.0 and int((fused != plain).sum()) <= 1


def test_seg_ce_fwd_of_an_empty_batch_zeroes_its_statistics(ops):
    """mv_seg_ce_fwd with B == 0 launches only the kernel that clears stats[0..3]."""
    from myrtle_vision.hip.lib import check, lib
    stats = torch.full((4,), 7.0, device="cuda")
    buf = torch.zeros(16, device="cuda")                  # small, labels, lse, pred, partials of an empty batch: never touched
    p = buf.data_ptr()
    check(lib().mv_seg_ce_fwd(p, p, p, p, p, stats.data_ptr(), 0, 8, 4, 4, 16, 16, ops._s()), "seg_ce_fwd")
    torch.cuda.synchronize()
    assert torch.equal(stats.cpu(), torch.zeros(4)) and (buf == 0).all()
