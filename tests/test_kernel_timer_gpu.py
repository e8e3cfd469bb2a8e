"""The kernel timer's records of one fused attention + MLP block step equal a literal list: the record names, shape labels and FLOP
counts that bench.py builds its roofline figure from (``summary()["gemm_nt_bf16"]``, ``["gemm_nt_bf16x6"]``, ``shape_summary()``).
With no timer installed nothing is recorded.  tools/diag/block_fingerprint.py prints the list for any pair of functional.py / ops.py.
D = 128, 2 heads of 64, MLP width 256, B = 2, T = 64: 128 rows, the smallest count at which ``x6_block_ok`` holds and the bf16 kernels
still see a full tile row."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, D, HEADS, MLP = 2, 64, 128, 2, 256

# (record name, shape label, algorithmic flops) in launch order: attn forward, mlp forward, mlp backward, attn backward
EXPECTED = {
    "bf16": [
        ('gemm_nt_bf16', 'fwd N384 K128 epi0', 12582912.0),
        ('gemm_nt_bf16', 'fwd N128 K128 epi2', 4194304.0),
        ('gemm_nt_bf16', 'fwd N256 K128 epi8', 8388608.0),
        ('gemm_nt_bf16', 'fwd N128 K256 epi2', 8388608.0),
        ('gemm_tn_bf16(+reduce+colsum)', 'dw N128 K256 bias1', 8388608.0),
        ('gemm_nt_bf16', 'dx N256 K128 epi9', 8388608.0),
        ('gemm_tn_bf16(+reduce+colsum)', 'dw N256 K128 bias0', 8388608.0),
        ('gemm_nt_bf16', 'dx N128 K256 epi0', 8388608.0),
        ('gemm_nt_bf16', 'dx N128 K128 epi0', 4194304.0),
        ('gemm_tn_bf16_group(+reduce)', 'dw x2', 16777216.0),
        ('gemm_nt_bf16', 'dx N128 K384 epi0', 12582912.0),
    ],
    "fp32": [
        ('gemm_nt_bf16x6', 'fwd N384 K128 epi0 S3', 12582912.0),
        ('gemm_nt_bf16x6', 'fwd N128 K128 epi2 S3', 4194304.0),
        ('gemm_nt_bf16x6', 'fwd N256 K128 epi0 S3', 8388608.0),
        ('gemm_nt_bf16x6', 'fwd N128 K256 epi2 S3', 8388608.0),
        ('gemm_tn_bf16x6', 'dw N128 K256', 8388608.0),
        ('gemm_nt_bf16x6', 'dx N256 K128 epi0 S3', 8388608.0),
        ('gemm_tn_bf16x6', 'dw N256 K128', 8388608.0),
        ('gemm_nt_bf16x6', 'dx N128 K256 epi0 S3', 8388608.0),
        ('gemm_tn_bf16x6', 'dw N128 K128', 4194304.0),
        ('gemm_nt_bf16x6', 'dx N128 K128 epi0 S3', 4194304.0),
        ('gemm_tn_bf16x6', 'dw N384 K128', 12582912.0),
        ('gemm_nt_bf16x6', 'dx N128 K384 epi0 S3', 12582912.0),
    ],
}
BENCH_KEY = {"bf16": "gemm_nt_bf16", "fp32": "gemm_nt_bf16x6"}


def _step(F, prec):
    gen = torch.Generator().manual_seed(5)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=gen) * k).cuda().requires_grad_(True)       # noqa: E731
    attn = [r(D, k=0.1), r(D, k=0.1), r(3 * D, D, k=0.08), r(3 * D, k=0.1), r(D, D, k=0.08), r(D, k=0.1)]
    mlp = [r(D, k=0.1), r(D, k=0.1), r(MLP, D, k=0.08), r(MLP, k=0.1), r(D, MLP, k=0.08), r(D, k=0.1)]
    x = r(B, T, D)
    F.chain_reset()
    out = F.mlp_block(F.attn_block(x, *attn, HEADS, (D // HEADS) ** -0.5, prec), *mlp, prec)
    out.sum().backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_timer_records_of_a_block_step(prec):
    from myrtle_vision.hip import functional as F, ops

    class Ordered(ops.KernelTimer):
        """``records`` and ``by_shape`` are keyed by name and by label: this keeps the order across keys."""
        def __init__(self):
            super().__init__()
            self.log = []

        def end(self, name, start, flops, shape=None):
            super().end(name, start, flops, shape=shape)
            if start is not None:
                self.log.append((name, shape, flops))

    timer = Ordered()
    assert ops.x6_block_ok(B * T, D, 3 * D, MLP)
    before = ops._timer
    ops.set_kernel_timer(timer)
    try:
        _step(F, prec)
        assert timer.log == EXPECTED[prec]
        # the two tables hold exactly these launches, each under its name and under its label
        for key, table in ((0, timer.records), (1, timer.by_shape)):
            want = {}
            for rec in EXPECTED[prec]:
                want.setdefault(rec[key], []).append(rec[2])
            assert {k: [f for _, _, f in v] for k, v in table.items()} == want
        summ = timer.summary()
        assert BENCH_KEY[prec] in summ and summ[BENCH_KEY[prec]]["launches"] > 0
        assert set(timer.shape_summary()) == {rec[1] for rec in EXPECTED[prec]}
        ops.set_kernel_timer(None)
        _step(F, prec)
        assert timer.log == EXPECTED[prec]
        assert sum(len(v) for v in timer.records.values()) == sum(len(v) for v in timer.by_shape.values()) == len(EXPECTED[prec])
    finally:
        ops.set_kernel_timer(before)
