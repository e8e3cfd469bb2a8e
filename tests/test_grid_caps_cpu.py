"""The launch caps of the grid-stride kernels, as a table that tests/test_grid_stride_gpu.py sizes its inputs from.

A grid-stride kernel launches at most ``cap`` workgroups; a workgroup takes ``per_group`` items per pass of the grid and an item is
``elems`` elements (or one row, one sample).  One pass therefore covers cap * per_group * elems elements, and an input has to be
larger than that before any thread runs its loop a second time.  The GPU tests assert that from this table; the test below reads
the cited .hip files and fails if a cited expression no longer carries the cited number, so a later change to a cap cannot
silently turn those tests back into one-pass tests.  It looks for the cap literals and for nothing else."""
import os
import re

import pytest

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")

# name: (source file, regular expression whose group 1 is the cap, cap, items per workgroup and pass, elements per item)
CAPS = {
    # ew_grid(): every elementwise / layout launch of elementwise.hip.  "v4": one 16-byte vector of four elements per thread
    "ew_v4": ("elementwise.hip", r"if \(g > (\d+)\) g = \1;\s+// 16 blocks per CU, grid-stride beyond", 4096, 256, 4),
    # one element (or one item: a pixel, a 16-byte group of a row, an output element) per thread
    "ew_s1": ("elementwise.hip", r"if \(g > (\d+)\) g = \1;\s+// 16 blocks per CU, grid-stride beyond", 4096, 256, 1),
    # ew_grid(total, 4): one wave per sample (cross_entropy_kernel) or per 1024-element chunk (quant_affine_i8_flat_kernel)
    "ew_w4": ("elementwise.hip", r"if \(g > (\d+)\) g = \1;\s+// 16 blocks per CU, grid-stride beyond", 4096, 4, 1),
    "softmax": ("gemm_f32.hip", r"if \(g > (\d+)\) g = \1;", 4096, 4, 1),                     # one wave per row, forward and backward
    "ce_soft": ("mixup.hip", r"int blocks = mv_cdiv\(B, 4\);\s+if \(blocks > (\d+)\) blocks = \1;", 4096, 4, 1),   # one wave per sample
    "distill": ("distill.hip", r"if \(blocks > (\d+)\) blocks = \1;", 4096, 4, 1),           # one wave per sample
    "ln_fwd": ("layernorm.hip", r"if \(grid > (\d+)\) grid = \1;", 2048, 4, 1),              # one wave per row; all three entry points
    "sumsq": ("elementwise.hip", r"constexpr int GN_PARTS = (\d+);", 1024, 256, 4),          # always this many workgroups
    "codes_vec": ("elementwise.hip", r"quant_affine_codes_vec_kernel<PRE\(\), T>>\(MV_HERE, rows < (\d+) \? \(int\)rows : \1,",
                  65536, 1, 1),                                                              # one row per workgroup
    "i8_rows": ("elementwise.hip", r"quant_affine_i8_kernel<PRE\(\), T>>\(MV_HERE, rows < (\d+) \? \(int\)rows : \1,",
                4096, 1, 1),                                                                 # one row per workgroup
    # colsum_parts(): at most this many partial rows, each over ceil(rows / parts) input rows -- 256 rows per part up to the cap
    "colsum_parts": ("gemm_bf16.hip", r"if \(p > (\d+)\) p = \1;", 256, 256, 1),
}


def one_pass(name):
    """Elements (rows, samples) that one pass of the capped grid covers."""
    _, _, cap, per_group, elems = CAPS[name]
    return cap * per_group * elems


def past_one_pass(name, tail):
    """The size the GPU tests use: one pass, five more workgroups' worth, and a ragged tail (three elements, or one row) -- some
    threads run two iterations, some one, and the scalar tail loop of the 16-byte kernels runs."""
    _, _, cap, per_group, elems = CAPS[name]
    return (cap + 5) * per_group * elems + tail


# The sizes the GPU tests use, written out: each must be what the table gives.
N_V4, N_S1, R_W4, R_LN, N_SUMSQ = 4_199_427, 1_049_859, 16_405, 8_213, 1_053_699


@pytest.mark.parametrize("name", sorted(CAPS))
def test_cited_cap_is_in_the_source(name):
    fname, pattern, cap, per_group, elems = CAPS[name]
    with open(os.path.join(CSRC, fname)) as f:
        found = re.findall(pattern, f.read())
    assert found, f"{fname}: no expression matches {pattern!r}"
    assert all(int(v) == cap for v in found), f"{fname}: {pattern!r} carries {found}, the table says {cap}"
    assert per_group > 0 and elems > 0


def test_sizes_are_one_pass_plus_five_workgroups_plus_a_ragged_tail():
    assert N_V4 == past_one_pass("ew_v4", 3) == 4_194_304 + 5_120 + 3
    assert N_S1 == past_one_pass("ew_s1", 3) == 1_048_576 + 1_280 + 3
    for name in ("ew_w4", "softmax", "ce_soft", "distill"):
        assert R_W4 == past_one_pass(name, 1) == 16_384 + 20 + 1
    assert R_LN == past_one_pass("ln_fwd", 1) == 8_192 + 20 + 1
    assert N_SUMSQ == past_one_pass("sumsq", 3) == 1_048_576 + 5_120 + 3
    for name, n in (("ew_v4", N_V4), ("ew_s1", N_S1), ("ew_w4", R_W4), ("softmax", R_W4), ("ln_fwd", R_LN), ("sumsq", N_SUMSQ)):
        assert n > one_pass(name)
