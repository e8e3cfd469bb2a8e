/* myrtle_vision HIP hot path -- C ABI (libmyrtle_vision_hip.so), gfx950 / MI355X only.
 *
 * The reference (MyrtleSoftware/myrtle-vision) has no FFI: its hot path is stock torch.nn
 * modules dispatching to ATen kernels.  Each entry point below replaces the ATen dispatch of
 * one reference call site (cited per function as <reference file>:<line>, relative to the
 * reference repo root, file src/myrtle_vision/models/vit.py unless another file is named).
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes; no torch types; device pointers unless stated
 *   - return 0 on success, a negative MV_ERR_* otherwise; never throw, never synchronise,
 *     never allocate (callers pass workspaces); work is enqueued on `stream`
 *   - re-entrant, no thread-local state (autograd calls backward from a worker thread); the ONLY process-global
 *     state is the kernel-variant overrides of mv_gemm_force_variant / mv_gemm_f32_force_fma / mv_attention_bwd_force (tuning / test hooks, atomic,
 *     default 0 = automatic): they change which kernel computes a product, never what is computed
 *   - "rows x dim" tensors are row-major; `ld*` are leading dimensions in ELEMENTS
 *   - dtype codes: MV_F32 / MV_BF16
 *   - MFMA entry points (mv_gemm_*_bf16, mv_attention_*) need 16-byte aligned pointers and
 *     leading dimensions that are multiples of 8 elements
 */
#ifndef MYRTLE_VISION_HIP_H
#define MYRTLE_VISION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mv_stream_t; /* hipStream_t */

enum { MV_F32 = 0, MV_BF16 = 1, MV_I8 = 2 /* mv_gemm_nt_i8 with MV_EPI_GELU_Q8 only */, MV_F16 = 3 /* IEEE half: mv_cast destination, mv_gemm_nt_bf16 output with MV_EPI_NONE */ };

enum {
  MV_OK = 0,
  MV_ERR_SHAPE = -1,       /* dimension constraint violated */
  MV_ERR_ALIGN = -2,       /* pointer / leading-dimension alignment */
  MV_ERR_LAUNCH = -3,      /* hipGetLastError() after launch */
  MV_ERR_UNSUPPORTED = -4, /* dtype / epilogue combination not built */
  MV_ERR_WORKSPACE = -5    /* workspace too small */
};

/* epilogues of the GEMM entry points */
enum {
  MV_EPI_NONE = 0,     /* C = acc (+ bias) */
  MV_EPI_GELU = 1,     /* out2 = acc + bias (pre-activation, optional); C = gelu_erf(acc + bias) */
  MV_EPI_RESIDUAL = 2, /* C = acc + bias + aux              (aux: fp32 [M, ld_aux]) */
  MV_EPI_DGELU = 3,    /* C = acc * gelu_erf'(aux)          (aux: pre-activation, dtype of A); bf16 kernel only: out2 (optional)
                          = fp32 [ceil(M/64), ld_out2] per-64-row column sums of C (bias-gradient partials) */
  MV_EPI_GELU_GRAD = 5, /* bf16 kernel only: C = gelu_erf(acc + bias), out2 (optional) = gelu_erf'(acc + bias): what the
                           backward needs, so that its epilogue is MV_EPI_MUL instead of re-evaluating erf */
  MV_EPI_MUL = 6,      /* bf16 kernel only: C = acc * aux (aux: dtype of A, e.g. the gelu' left by MV_EPI_GELU_GRAD);
                          out2 as MV_EPI_DGELU (per-64-row column sums of C) */
  MV_EPI_GELU_Q8 = 7,  /* mv_gemm_nt_i8 only: C (int8) = quint8 code - 128 of gelu_erf(acc + bias) under the NEXT layer's
                          quantiser (q_scale, q_zero_point): FeedForward's Linear -> GELU -> next Linear's QuantStub
                          (vit.py:48-51) without the fp32 hidden activations ever reaching memory */
  MV_EPI_GELU_GRAD8 = 8, /* as MV_EPI_GELU_GRAD with out2 as ONE BYTE per element (uint8 [M, ld_out2]): gelu' lies in
                            [-0.129, 1.129]; code = round(gelu' * 200) + 26: 0 and 1 are codes 26 and 226 exactly, |error| <= 0.0025 */
  MV_EPI_MUL8 = 9,       /* as MV_EPI_MUL with aux = those codes (uint8 [M, ld_aux]): C = acc * ((code - 26) * 0.005) */
  MV_EPI_SPLIT_DGELU = 10, /* mv_gemm_nt_bf16 with C bf16 [M, aux_i * N] (aux_i = 3 | 6): the bf16 PIECES (mv_split2_bf16 / mv_split3_bf16,
                              role 0, segments N apart) of acc * gelu_erf'(aux), aux fp32 [M, ld_aux]; out2 as MV_EPI_DGELU.  The
                              fc2 input gradient of the split-operand modes leaves as the operand of fc1's dW / dX products: no fp32
                              tensor, no split pass.  Whole 256 x 256 tiles only (M % 256 == N % 256 == 0) */
  MV_EPI_SPLIT_GELU = 11,  /* likewise: out2 = acc + bias (fp32 pre-activation [M, ld_out2], required), C = the pieces of
                              gelu_erf(acc + bias): fc1 of the split-operand modes */
  MV_EPI_EMBED = 4     /* patch-embedding: row m of the GEMM is patch (m % aux_i) of image (m / aux_i);
                          C row = img*(aux_i+1) + 1 + patch;  C = acc + bias + aux[1 + patch]  (aux: fp32 [aux_i+1, N]) */
};

int mv_version(void);
const char* mv_error_string(int code);
/* number of bytes of workspace mv_gemm_tn_bf16 / mv_layernorm_bwd want for these sizes */
size_t mv_gemm_tn_workspace_bytes(int M, int N, int Kc);
/* Tuning / test hook (no reference counterpart): force a kernel variant for the following mv_gemm_nt_bf16 (0 auto | 128 | 2564 ring |
 * 2568 8-phase | 25680 8-phase without the half-item tail | 3000 / 3002 automatic dispatch with the 8-phase kernel's column bands
 * off / on | 3100 / 3102 the same with the 8-phase kernel forced) and mv_gemm_tn_bf16 (0 auto | 128 | 256 ring; 1000 more, i.e.
 * 1000 | 1128 | 1256: the same, and mv_gemm_tn_bf16_group runs its items one by one) calls of this
 * process; a forced variant that cannot run a shape (alignment of K) falls back to the automatic choice.  Results are identical up
 * to fp32 summation order (bands on / off: bit for bit). */
int mv_gemm_force_variant(int nt_variant, int tn_variant);
size_t mv_layernorm_bwd_workspace_bytes(int rows, int dim);

/* ---- LayerNorm: nn.LayerNorm(dim), eps 1e-5 -- vit.py:37,41 (PreNorm), :332,:353 (decoder norms) ----
 * x: fp32 [rows, dim] with row stride ldx (lets the decoder read x[:,0] / x[:,1:] in place);
 * y: y_dtype [rows, dim] dense; mean/rstd: fp32 [rows] (saved for backward). */
int mv_layernorm_fwd(const float* x, long ldx, const float* gamma, const float* beta, void* y, int y_dtype,
                     float* mean, float* rstd, int rows, int dim, float eps, mv_stream_t stream);
/* The same LayerNorm with the output leaving as the bf16 pieces of the split-operand Linear products (nseg = 6: mv_split3_bf16's
 * role-0 side-by-side layout [rows, 6 * dim], nseg = 3: mv_split2_bf16's [rows, 3 * dim]); bit-identical to mv_layernorm_fwd (fp32)
 * followed by the split, without the fp32 tensor in between.  dim <= 1024. */
int mv_layernorm_fwd_split(const float* x, long ldx, const float* gamma, const float* beta, void* y_split, int nseg, float* mean,
                           float* rstd, int rows, int dim, float eps, mv_stream_t stream);
/* dx[rows, dim] (fp32, row stride lddx) = dLN(dy) (+ dx_add if non-null, same layout as dx; may alias dx);
 * dgamma/dbeta: fp32 [dim], overwritten (accumulate=0) or added to (accumulate=1).
 * Optional fused by-products for the consumer of dx in the backward chain (both may be NULL):
 *   dx_bf16  : bf16 [rows, dim] dense copy of dx (the MFMA operand of the next block's dX/dW products);
 *   dx_colsum: fp32 [dim] = sum over rows of dx (that block's output-projection bias gradient), overwritten. */
int mv_layernorm_bwd(const void* dy, int dy_dtype, const float* x, long ldx, const float* gamma,
                     const float* mean, const float* rstd, const float* dx_add, float* dx, long lddx,
                     float* dgamma, float* dbeta, int accumulate, float* workspace, size_t workspace_bytes,
                     int rows, int dim, void* dx_bf16, float* dx_colsum, mv_stream_t stream);
/* The same backward with dx ALSO leaving as the bf16 pieces of the split-operand products (dx_split [rows, nseg * dim], nseg = 3 | 6,
 * mv_split2_bf16 / mv_split3_bf16 role 0): what the consumer of dx in backward order feeds its dW / dX products, without a split pass. */
int mv_layernorm_bwd_split(const void* dy, int dy_dtype, const float* x, long ldx, const float* gamma, const float* mean,
                           const float* rstd, const float* dx_add, float* dx, long lddx, float* dgamma, float* dbeta, int accumulate,
                           float* workspace, size_t workspace_bytes, int rows, int dim, void* dx_split, int nseg, float* dx_colsum,
                           mv_stream_t stream);

/* ---- dense contractions on MFMA (bf16 in, fp32 accumulate) ----
 * nn.Linear forward  y = x W^T + b : patch_to_embedding :278, to_qkv :86, to_out :98, net.0/net.3 :48-51,
 * decoder.linear :333/:354.   C[M,N] = A[M,K] . B[N,K]^T  (both operands K-contiguous).
 * The same entry point computes the input gradient dX = dY . W with B = W^T[K_in, N_out] (a transposed
 * bf16 copy the host keeps), i.e. autograd's mm for AddmmBackward.
 * Requirements: K % 8 == 0 is NOT required, but rows must be readable (and zero) up to round_up(K, 8). */
int mv_gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int c_dtype, int M, int N,
                    int K, const float* bias, int epilogue, const void* aux, int ld_aux, int aux_i, void* out2,
                    int ld_out2, mv_stream_t stream);
/* the same with C = alpha * (A . B^T) (+ bias, epilogue): the integer-code products of the converted int8 path
 * (mv_quant_affine_codes), where alpha = scale_activation * scale_weight.  Serves QFormat.PyTorchINT8 after convert()
 * (utils/quantize.py:230-251, 329-338: torch.quantization.convert -> quantized::linear, which does not run in the
 * reference; classification/test_quantize.py:26-34,145-156 is the caller). */
int mv_gemm_nt_bf16_scaled(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int c_dtype, int M, int N,
                           int K, float alpha, const float* bias, int epilogue, const void* aux, int ld_aux, int aux_i,
                           void* out2, int ld_out2, mv_stream_t stream);
/* weight gradient  dW[M,N] (fp32) (+)= A[Kc,M]^T . B[Kc,N]  (A = dY, B = X; contraction over tokens) --
 * autograd's mm(dY^T, X) for every nn.Linear above.  Split over Kc into fp32 slabs in `workspace`,
 * reduced deterministically.  colsum (optional, fp32 [M]) (+)= column sums of A = bias gradient. */
int mv_gemm_tn_bf16(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int Kc,
                    int accumulate, float* colsum, float* workspace, size_t workspace_bytes, mv_stream_t stream);
/* Up to 4 weight gradients over the SAME Kc token rows (the to_out and to_qkv products of one attention block) in one launch:
 * C_i[M_i, N_i] = A_i[Kc, M_i]^T . B_i[Kc, N_i], no accumulate, no colsum.  `items` is a HOST array, read before the call returns.
 * The split count is chosen for the items' tiles together and is the same for all of them; one reduce sums every item's slabs
 * in split order (deterministic).  When Kc is not a multiple of 32, an item alone would not take the 256-tile kernel, or the TN
 * force code is 1000 + family, the items run one after another exactly as mv_gemm_tn_bf16 calls (same bits as those).  A
 * one-item group computes what mv_gemm_tn_bf16 computes, bit for bit. */
typedef struct mv_tn_item {
  const void* A;
  int lda;
  const void* B;
  int ldb;
  float* C;
  int ldc;
  int M;
  int N;
} mv_tn_item;
size_t mv_gemm_tn_group_workspace_bytes(const mv_tn_item* items, int n_items, int Kc);
int mv_gemm_tn_bf16_group(const mv_tn_item* items, int n_items, int Kc, float* workspace, size_t workspace_bytes,
                          mv_stream_t stream);

/* ---- generic fp32 contraction (exact-parity mode, odd shapes, materialised attention) ----
 * C[b1,b2][m,n] = sum_k A[b1,b2][m,k] * B[b1,b2][k,n] with arbitrary element strides; same epilogues
 * (aux/out2 are fp32).  alpha scales the accumulator before the epilogue; accumulate adds into C. */
int mv_gemm_f32(const float* A, long sa_m, long sa_k, long sa_b1, long sa_b2, const float* B, long sb_k, long sb_n,
                long sb_b1, long sb_b2, float* C, long sc_m, long sc_n, long sc_b1, long sc_b2, int M, int N, int K,
                int nb1, int nb2, float alpha, int accumulate, const float* bias, int epilogue, const float* aux,
                long ld_aux, int aux_i, float* out2, long ld_out2, mv_stream_t stream);
/* out[i] (+)= sum_s slabs[s * stride + i], s in fixed order: the deterministic reduce of a product whose contraction was
 * split over mv_gemm_f32's batch dimension (dW = dY^T X has 50 432 contraction rows and only 36-144 output tiles) */
int mv_sum_slabs(const float* slabs, long stride, int S, float* out, long n, int accumulate, mv_stream_t stream);
/* out[i] = (add ? add[i] : 0) + sum over s of slabs[s * stride + i]; add may alias out */
int mv_sum_slabs_add(const float* slabs, long stride, int S, const float* add, float* out, long n, mv_stream_t stream);
/* Test / tuning hook (no reference counterpart; the second piece of process-global state next to mv_gemm_force_variant):
 * 1 = mv_gemm_f32 runs its FMA kernel, 0 (default; MV_GEMM_F32=fma in the environment starts with 1) = the f32-input MFMA
 * kernels, 2 = matrix cores but only the generic (any stride, any size) kernel.  All compute the same k-ordered fmaf chain
 * per output: results are bit-identical. */
int mv_gemm_f32_force_fma(int on);

/* ---- fused multi-head self-attention core -- Attention.forward vit.py:87-96 ----
 * qkv: bf16 [B, N, 3, H, 64] (the to_qkv output, feature order [q|k|v][head][dh], vit.py:87-90);
 * out: bf16 [B, N, H*64] = (softmax(q k^T * scale) v).transpose(1,2).reshape(B,N,C);  lse: fp32 [B,H,N].
 * dim_head must be 64 (all shipped configs; ViT default dim_head=64, vit.py:178); N <= 320. */
int mv_attention_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, float scale, mv_stream_t stream);
/* dqkv: bf16 [B, N, 3, H, 64]; dout/out: bf16 [B, N, H*64].  colsum (optional): fp32 [B, 3*H*64], row b = column sums
 * of image b's dqkv rows (fp32 accumulators, before the bf16 rounding) -- summed over b they are to_qkv's bias gradient,
 * so no separate pass over dqkv is needed for it. */
int mv_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* colsum,
                     int B, int N, int H, float scale, mv_stream_t stream);
/* The same attention core for any 1 <= N <= 8192 (Attention.forward vit.py:87-96; the position table interpolated to larger
 * grids, vit.py:216-218,292-302, gives 577 tokens at 384^2, 1 025 at 512^2): key-tiled kernels that stream K / V (or Q / dO)
 * through LDS in 64-row blocks with an online softmax, so no [N, N] tensor exists.  Layouts, alignment (16 bytes for every
 * bf16 tensor), lse and colsum as mv_attention_fwd / mv_attention_bwd; the same rounding points (P and dS rounded to bf16 before
 * their products, fp32 accumulation, outputs rounded once).  Backward: delta_ws is a caller-provided fp32 workspace of
 * B * H * N floats (it receives rowsum(dout * out)); colsum here sums the bf16 dqkv rows in a fixed order.  Deterministic: no
 * atomics, every output has one owner.  ops.attention_fwd / _bwd take these for N > 320 and the kernels above otherwise. */
int mv_attention_fwd_long(const void* qkv, void* out, float* lse, int B, int N, int H, float scale, mv_stream_t stream);
int mv_attention_bwd_long(const void* qkv, const void* out, const void* dout, const float* lse, float* delta_ws, void* dqkv,
                          float* colsum, int B, int N, int H, float scale, mv_stream_t stream);
/* The bf16 attention core for head widths other than 64 (Attention.forward vit.py:85-99; dim_head is a constructor argument of the
 * reference's ViT / Attention and only heads * dim_head is fixed by the model width): dim_head 32 or 128, any 1 <= N <= 8192.
 * Key-tiled kernels like mv_attention_fwd_long / _bwd_long with the same rounding points (P and dS rounded to bf16 before their
 * products, fp32 softmax and accumulation, outputs rounded once) and no [N, N] tensor.  qkv: bf16 [B, N, 3, H, dim_head];
 * out / dout: bf16 [B, N, H * dim_head]; lse: fp32 [B, H, N], natural-log units; dqkv as qkv; every bf16 tensor 16-byte aligned.
 * delta_ws: caller-provided fp32 workspace of B * H * N floats (receives rowsum(dout * out)).  colsum (nullable): fp32
 * [B, 3 * H * dim_head], per-image column sums of the bf16 dqkv rows in a fixed order (to_qkv's bias-gradient partials).
 * Deterministic: no atomics, every output has one owner.  N outside 1 .. 8192: MV_ERR_SHAPE; a misaligned pointer: MV_ERR_ALIGN;
 * any other dim_head: MV_ERR_UNSUPPORTED (64: mv_attention_fwd / _fwd_long) -- nothing is launched in these cases. */
int mv_attention_fwd_dh(const void* qkv, void* out, float* lse, int B, int N, int H, int dim_head, float scale,
                        mv_stream_t stream);
int mv_attention_bwd_dh(const void* qkv, const void* out, const void* dout, const float* lse, float* delta_ws, void* dqkv,
                        float* colsum, int B, int N, int H, int dim_head, float scale, mv_stream_t stream);
/* The attention core of precision "bf16x3" (vit.py:87-96 between fp32 tensors): the fused kernels above on IEEE-half operands with
 * fp32 accumulation, softmax and OUTPUTS; N <= 288 (longer: mv_attention_fwd_long_f16 below; N <= 208: the 13-key-tile kernels; above: the two-pass kernels of the 257-token case).  qkv16: half [B, N, 3, H, 64] (mv_cast to MV_F16 of the fp32 to_qkv output);
 * out / lse as mv_attention_fwd but out is fp32.  Backward: mv_attention_bwd_prep_f16 turns the fp32 dout [B, N, H*64] into half
 * scaled, per (image, head), by a power of two s (the slice's largest magnitude -> [2^7, 2^8): gradients lie below half's normal
 * range otherwise), leaves s in gscale[b * H + h] (device, fp32 [B * H]) and delta[b, h, n] = sum_d half(dout * s) * out.
 * mv_attention_bwd_f16 then writes dqkv with s divided out (exactly): nseg = 0: fp32 [B, N, 3, H, 64]; nseg = 3 / 6: the bf16 pieces of
 * the split-operand products ([B * N, nseg * 3 * H * 64], mv_split2_bf16 / mv_split3_bf16 role 0) -- the dY operand of to_qkv's dW
 * and dX products without an fp32 tensor and a split pass; colsum (optional) as mv_attention_bwd. */
int mv_attention_fwd_f16(const void* qkv16, float* out, float* lse, int B, int N, int H, float scale, mv_stream_t stream);
int mv_attention_bwd_prep_f16(const float* dout, const float* out, void* dout16, float* delta, float* gscale, int B, int N, int H,
                              mv_stream_t stream);
int mv_attention_bwd_f16(const void* qkv16, const void* dout16, const float* delta, const float* lse, const float* gscale,
                         void* dqkv, int nseg, float* colsum, int B, int N, int H, float scale, mv_stream_t stream);
/* The same half-operand core for any 1 <= N <= 8192 (precision "bf16x3h" at 384^2 fine-tuning, 577 tokens, and 512^2 segmentation,
 * 1 025): the key-tiled kernels of mv_attention_fwd_long / _bwd_long on IEEE half, so no [N, N] tensor exists.  Arguments, layouts,
 * alignment and the roundings as mv_attention_fwd_f16 / mv_attention_bwd_f16 (dout16, delta and gscale from
 * mv_attention_bwd_prep_f16, which takes any N).  colsum_ws: a caller-provided fp32 workspace of B * ceil(N / 128) * 3 * H * 64
 * floats, needed only with colsum: every 128-row block of keys and of queries leaves the column sums of its fp32 dqkv rows there,
 * and a fixed-order pass adds them into colsum.  Deterministic: no atomics, every output has one owner.  ops.attention_fwd_f16 /
 * _bwd_f16 take these for N > 288 and the kernels above otherwise. */
int mv_attention_fwd_long_f16(const void* qkv16, float* out, float* lse, int B, int N, int H, float scale, mv_stream_t stream);
int mv_attention_bwd_long_f16(const void* qkv16, const void* dout16, const float* delta, const float* lse, const float* gscale,
                              void* dqkv, int nseg, float* colsum, float* colsum_ws, int B, int N, int H, float scale,
                              mv_stream_t stream);
/* Test / tuning hook (process-global, atomic, like mv_gemm_force_variant): backward kernel for the following
 * mv_attention_bwd calls -- 0 auto (N <= 208: 4; N <= 288: 2; else 8), 4 = dS exchanged through LDS (N <= 208), 5 = the same
 * with two waves of 512 registers per workgroup (192 < N <= 208; equal results up to the placement of the softmax scale), 2 = two
 * barrier-free passes (N <= 288), 8 = the eight-wave kernel (N <= 320).  A variant that cannot take the length falls back
 * to auto. */
int mv_attention_bwd_force(int variant);
/* The same for mv_attention_fwd: 0 auto (N <= 208: 3, else 1), 3 = 13 key tiles in 53 KB of LDS, three workgroups per CU (N <= 208),
 * 1 = one 16-query tile per wave and pass, 2 = a PAIR of query
 * tiles per wave and pass (every K / V^T fragment read from LDS feeds two MFMAs; N <= 224, else falls back to 1). */
int mv_attention_fwd_force(int variant);
/* The same attention core in EXACT fp32 arithmetic on the f32-input matrix cores, forward only: qkv fp32 [B, N, 3, H, 64],
 * out fp32 [B, N, H*64]; N <= 272.  For the paths that need fp32 values and no gradient (converted PyTorchINT8 model,
 * precision="fp32" evaluation): same products and sums as mv_gemm_f32 + mv_softmax_fwd + mv_gemm_f32 up to summation order,
 * without the [B, H, N, N] probabilities. */
int mv_attention_fwd_f32(const float* qkv, float* out, int B, int N, int H, float scale, mv_stream_t stream);

/* ---- row softmax for the materialised attention path (fp32): attn.softmax(dim=-1) vit.py:93 ---- */
int mv_softmax_fwd(const float* x, float* y, long rows, int cols, float scale, mv_stream_t stream);
/* dx = scale * y * (dy - sum(dy*y)) */
int mv_softmax_bwd(const float* y, const float* dy, float* dx, long rows, int cols, float scale, mv_stream_t stream);

/* ---- patchify: vit.py:271-275  (B,C,H,W) fp32 -> (B*gh*gw, p*p*C) out_dtype, k = (py*p+px)*C + c ---- */
int mv_patchify(const float* img, void* out, int out_dtype, int B, int C, int H, int W, int p, mv_stream_t stream);
/* cls row of the embedding: x[b, 0, :] = cls[:] + pos[0, :]  (vit.py:283-290,305-310); x fp32 [B, T, D] */
int mv_embed_cls(const float* cls, const float* pos, float* x, int B, int T, int D, mv_stream_t stream);
/* backward of the embedding assembly: dpos[t, :] (+)= sum_b dx[b, t, :];  dcls[:] (+)= sum_b dx[b, 0, :] */
int mv_embed_bwd(const float* dx, float* dpos, float* dcls, int accumulate, int B, int T, int D, mv_stream_t stream);
/* mv_embed_bwd and mv_gather_patch_rows in one pass over dx (vit.py:271-311 backward): dpos / dcls as mv_embed_bwd (either may be NULL; written, not
 * accumulated) and dy = rows 1..T-1 of every image in dy_dtype (NULL: skipped) -- the dY operand of the patch GEMM's dW product.
 * D % 4 == 0, pointers 16-byte aligned. */
int mv_embed_bwd_gather(const float* dx, void* dy, int dy_dtype, float* dpos, float* dcls, int B, int T, int D,
                        mv_stream_t stream);
/* gather rows 1..T-1 of every image: dst[b*(T-1)+t-1, :] = (dtype) src[b, t, :]  (dY for the patch GEMM) */
int mv_gather_patch_rows(const float* src, void* dst, int dst_dtype, int B, int T, int D, mv_stream_t stream);

/* ---- positional-embedding resize: vit.py:292-302  F.interpolate(mode="bicubic", align_corners=False) on the (1, D, sh, sw) view ----
 * pos / dpos fp32 [1 + sh*sw, D], out / dout fp32 [1 + gh*gw, D], token-major (the reference's transposes are index arithmetic).  Row 0
 * (the cls slot) passes through; row 1 + y*gw + x is the grid resized to (gh, gw) as torch's upsample_bicubic2d defines it: per axis
 * src = (dst + 0.5) * (in / out) - 0.5 (not clamped), taps floor(src) - 1 .. + 2 with indices clamped to [0, in - 1], cubic-convolution
 * weights with A = -0.75, all in fp32; four taps without antialiasing when downscaling too; bit-exact copy when the grids are equal.
 * Taps and weights are computed inside the kernels: no table comes from the host.
 * D % 4 == 0 and every side positive (MV_ERR_SHAPE); sh, sw, gh, gw <= 1024 each (MV_ERR_UNSUPPORTED: the backward keeps one weight per
 * target row and column in LDS); pointers non-NULL and 16-byte aligned (MV_ERR_ALIGN).  Nothing is launched in these cases. */
int mv_pos_resize_fwd(const float* pos, float* out, int sh, int sw, int gh, int gw, int D, mv_stream_t stream);
/* the exact transpose: dpos[1 + q, :] (+)= sum_p R[p, q] * dout[1 + p, :], dpos[0, :] (+)= dout[0, :]; taps clamped onto a border cell all land
 * on that cell.  accumulate != 0 adds into dpos, otherwise every row of dpos is overwritten (rows no target touches with 0).  A gather per
 * source cell with a fixed summation order: deterministic, no atomics on floats.  Same argument checks as mv_pos_resize_fwd. */
int mv_pos_resize_bwd(const float* dout, float* dpos, int accumulate, int sh, int sw, int gh, int gw, int D, mv_stream_t stream);

/* ---- casts / layout ---- */
/* dst (dst_dtype) = src (src_dtype), n elements */
int mv_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, mv_stream_t stream);
/* fp32 -> three bf16 pieces for the "bf16x6" fp32 product (the fp32 arithmetic mode of nn.Linear, vit.py:48-51,72-74, on
 * the bf16 matrix cores): x = p0 + p1 + p2 to 2^-26 |x|; writes the six segments of one operand, ``seg`` elements apart,
 * in the order role 0 (left operand): p0 p0 p1 p0 p1 p2, role 1 (right operand): p0 p1 p0 p2 p1 p0, so that a bf16 product
 * contracting over all six segments equals the fp32 product to 2^-25 relative.  out row stride ldo; seg = cols with
 * ldo = 6 * cols lays the segments side by side along the contraction axis of an NT product, seg = rows * ldo stacks
 * them along the rows (TN product).  cols, ldx, ldo, seg multiples of 4; x and out 16-byte aligned. */
int mv_split3_bf16(const float* x, long ldx, void* out, long ldo, long seg, long rows, int cols, int role,
                   mv_stream_t stream);
/* The role-0 side-by-side split (out [rows, 6 * cols] bf16) of v, behind a producer's last elementwise step: op 0: v = x;
 * op 1: v = gelu(x) (nn.GELU, vit.py:49: fc1's activation as the fc2 operand, the fp32 activation never stored); op 2:
 * v = x * gelu'(h) (fc2's dX times the activation derivative).  colsum (optional, fp32 [cols]) receives the column sums of v
 * = the bias gradient of the Linear that v is the output gradient of (deterministic two-stage sum; workspace of
 * mv_split3_ex_workspace_bytes(rows, cols) bytes, needed only with colsum). */
size_t mv_split3_ex_workspace_bytes(long rows, int cols);
int mv_split3_bf16_ex(const float* x, long ldx, const float* h, long ldh, int op, void* out, long rows, int cols,
                      float* colsum, float* workspace, size_t workspace_bytes, mv_stream_t stream);
/* K-split form of mv_gemm_nt_bf16 for products with few output tiles and a long contraction (the bf16x6 products with a
 * 768-wide output at batch 64: 150 tiles of 256x256 on 256 CUs): slabs[s] (fp32 [M, N], dense, s < splits) = A[:, slice s]
 * B[:, slice s]^T, the bias added to slab 0; sum with mv_sum_slabs_add.  K % (128 * splits) == 0, N % 4 == 0. */
int mv_gemm_nt_bf16_ksplit(const void* A, int lda, const void* B, int ldb, float* slabs, int M, int N, int K, int splits,
                           const float* bias, mv_stream_t stream);
/* dW of an fp32 nn.Linear as a bf16x6 product: A6 = the role-0 side-by-side split (seg = cols, ldo = 6 * cols) of dY
 * [rows, M], B6 = that of X [rows, N]; C[M, N] (fp32, row stride ldc) = dY^T X to fp32 accuracy.  The kernel addresses the
 * six piece pairings inside the two buffers itself, so the splits made for the dX / forward products are reused as they
 * are.  M, N multiples of 8, rows a multiple of 32; workspace as mv_gemm_tn_workspace_bytes(M, N, 6 * rows). */
int mv_gemm_tn_bf16_x6(const void* A6, const void* B6, float* C, int ldc, int M, int N, int rows, float* workspace,
                       size_t workspace_bytes, mv_stream_t stream);
/* "bf16x3": the fp32 products of nn.Linear (vit.py:48-51,72-74,86) to 2^-16 relative -- inside BASELINE's 1e-3 end to end -- at
 * half the matrix-core work of bf16x6 (``precision="bf16x3"``).  Each operand as TWO bf16 pieces p0 = bf16(x), p1 = bf16(x - p0),
 * three segments in the order role 0: p0 p0 p1, role 1: p0 p1 p0 (the first three of mv_split3_bf16's six), so a bf16 product
 * over the 3 * K contraction is a0 b0 + a0 b1 + a1 b0.  Same argument meaning as mv_split3_bf16 / mv_split3_bf16_ex (the _ex
 * form writes [rows, 3 * cols]; workspace as mv_split3_ex_workspace_bytes) / mv_gemm_tn_bf16_x6 (A3 [rows, 3 M], B3 [rows, 3 N],
 * workspace as mv_gemm_tn_workspace_bytes(M, N, 3 * rows)). */
int mv_split2_bf16(const float* x, long ldx, void* out, long ldo, long seg, long rows, int cols, int role,
                   mv_stream_t stream);
int mv_split2_bf16_ex(const float* x, long ldx, const float* h, long ldh, int op, void* out, long rows, int cols,
                      float* colsum, float* workspace, size_t workspace_bytes, mv_stream_t stream);
/* The right-operand pieces of an nn.Linear weight w [R = out, C = in] (fp32, dense) for BOTH of its split-operand products from
 * one read: fwd [R, nseg * C] = mv_split2/3_bf16(w, role 1) (y = x W^T, vit.py:48-51,86,98) and dx [C, nseg * R] = the same of w^T
 * (dx = dy W); either may be NULL.  nseg = 3 | 6; R and C even.  Replaces a transposed fp32 copy + two split passes per weight and
 * optimizer step. */
int mv_weight_split(const float* w, void* fwd, void* dx, int R, int C, int nseg, mv_stream_t stream);
int mv_gemm_tn_bf16_x3(const void* A3, const void* B3, float* C, int ldc, int M, int N, int rows, float* workspace,
                       size_t workspace_bytes, mv_stream_t stream);
/* weight prep for the MFMA path: w fp32 [R, C] -> w_bf16 [R, ldw] and wt_bf16 [C, ldt] (transposed), pads zeroed;
 * either output may be NULL */
int mv_weight_prep(const float* w, void* w_bf16, int ldw, void* wt_bf16, int ldt, int R, int C, mv_stream_t stream);
/* the same for many weights in one launch (after an optimizer step every nn.Linear weight of the model is stale:
 * vit.py:72-74,86,48-51 x depth).  ``items_device``: DEVICE array of ``count`` items sorted by first_block; item i covers
 * blocks [first_block, first_block + tiles_x * tiles_y) with tiles_x = ceil(max(C, ldw) / 64), tiles_y = ceil(max(R, ldt)
 * / 64); first_block of item 0 is 0 and total_blocks is the sum.  Both outputs of every item are required; ldw and
 * ldt even, w 8-byte and the outputs 4-byte aligned. */
typedef struct mv_weight_prep_item {
  const float* w;
  void* w_bf16;
  void* wt_bf16;
  int ldw, ldt, R, C;
  int tiles_x, first_block;
} mv_weight_prep_item;
int mv_weight_prep_batch(const mv_weight_prep_item* items_device, int count, int total_blocks, mv_stream_t stream);
/* column sums (bias gradient): out[c] (+)= sum_r x[r, c]; x dtype x_dtype [rows, ld] */
int mv_colsum(const void* x, int x_dtype, long ld, float* out, int accumulate, long rows, int cols, float* workspace,
              size_t workspace_bytes, mv_stream_t stream);
/* y = gelu(x) and dx = dy * gelu'(x) (unfused forms, fp32/bf16) */
int mv_gelu_fwd(const void* x, void* y, int dtype, long n, mv_stream_t stream);
int mv_gelu_bwd(const void* x, const void* dy, void* dx, int dtype, long n, mv_stream_t stream);
/* out = a + b (fp32), n elements: Residual.res_add vit.py:27 in the unfused path */
int mv_add_f32(const float* a, const float* b, float* out, long n, mv_stream_t stream);

/* ---- fake quantisation (QPyTorch path): utils/quantize.py:46-72,84 ----
 * fp32 in/out, nearest rounding; float format (exp, man) or fixed point (wl, fl); in place allowed */
int mv_quant_float(const float* x, float* y, long n, int exp_bits, int man_bits, mv_stream_t stream);
int mv_quant_fixed(const float* x, float* y, long n, int wl, int fl, int clamp, int symmetric, mv_stream_t stream);
/* per-tensor affine fake-quant (MinMaxObserver qparams, utils/quantize.py:242-249) */
int mv_quant_affine(const float* x, float* y, long n, float scale, int zero_point, int qmin, int qmax,
                    mv_stream_t stream);
/* (utils/quantize.py:242-249: MinMaxObserver quint8 affine activations / qint8 symmetric weights)
 * integer codes of the affine quantiser, re-centred: codes[r, c] = clamp(rint(x / scale) + zp, qmin, qmax) - zp as bf16
 * (exact: |code| <= 256), rows ld elements apart with zeroed padding -- an MFMA operand whose products with another
 * code tensor, accumulated in fp32, are the exact integer dot products of real int8 inference.
 * x_dtype: MV_F32 or MV_BF16 (the fused attention kernel's output).  pre_op 1: x is passed through GELU (erf form) first -- FeedForward's nn.GELU between its two quantised Linears
 * (vit.py:48-51) without the fp32 round trip; 0: none. */
int mv_quant_affine_codes(const void* x, int x_dtype, void* codes, long rows, int cols, int ld, float scale, int zero_point,
                          int qmin, int qmax, int pre_op, mv_stream_t stream);
/* float_quantize(exp 5, man 10) written as IEEE half (exact: every value of the format is a half), and the NT product of two
 * such operands on v_mfma_f32_16x16x32_f16 with fp32 accumulation: the FORWARD products of the FP16_16 / FP16_32 formats
 * (quantize.py:253-327: both the activation stub and weight_fake_quant round to (5, 10)), which the reference computes as an
 * fp32 GEMM of the same values.  A [M, lda], B [N, ldb] half, K % 128 == 0; C fp32; epilogues MV_EPI_NONE / MV_EPI_RESIDUAL. */
int mv_quant_float_f16(const float* x, void* y, long n, mv_stream_t stream);
int mv_gemm_nt_f16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const float* bias,
                   int epilogue, const void* aux, int ld_aux, void* out2, int ld_out2, mv_stream_t stream);
/* the same quantiser writing int8 codes q - 128 (quint8: qmin 0, qmax 255) for mv_gemm_nt_i8; ld = row stride in BYTES
 * (multiple of 16), columns [cols, ld) zero-filled */
int mv_quant_affine_i8(const void* x, int x_dtype, void* codes, long rows, int cols, int ld, float scale, int zero_point,
                       int pre_op, mv_stream_t stream);
/* int8 x int8 -> int32 NT product on v_mfma_i32_16x16x64_i8 with the affine bookkeeping in the epilogue (config 5; build-
 * defined: the reference's converted PyTorchINT8 path, quantize.py:230-251 + classification/test_quantize.py:109, does not run):
 *   C[m][n] = alpha * ( sum_k A8[m][k] * B8[n][k] + icorr[n] ) + bias[n]  (+ aux[m][n] for MV_EPI_RESIDUAL)
 * With A8 = q_x - 128, B8 = q_w and icorr[n] = (128 - zero_point_x) * sum_k q_w[n][k] the bracket is the exact integer dot
 * product of (q_x - zero_point_x) and q_w; alpha = scale_x * scale_w.  A8 [M, lda], B8 [N, ldb] int8, strides in bytes
 * (multiples of 16), K % 256 == 0; C fp32 or bf16; epilogues MV_EPI_NONE / MV_EPI_RESIDUAL (fp32) / MV_EPI_GELU_Q8 (C int8
 * [M, ldc bytes], c_dtype MV_I8, M % 256 == N % 256 == 0; q_scale / q_zero_point: the next layer's quantiser). */
int mv_gemm_nt_i8(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int c_dtype, int M, int N, int K,
                  float alpha, const float* bias, const int* icorr, int epilogue, const void* aux, int ld_aux,
                  float q_scale, int q_zero_point, mv_stream_t stream);
/* The same fp32 core for TRAINING in precision="fp32" (vit.py:92-96 forward and its autograd backward), still without the
 * [B, H, N, N] tensors: the forward also leaves lse[b, h, n] = log sum_j exp(scale q_n . k_j) (fp32 [B, H, N]); the backward
 * recomputes the probabilities from it and returns dqkv (fp32, qkv's layout) from qkv, out (the forward's result), dout.
 * N <= 272, dim_head 64. */
int mv_attention_fwd_f32_lse(const float* qkv, float* out, float* lse, int B, int N, int H, float scale, mv_stream_t stream);
int mv_attention_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int N,
                         int H, float scale, mv_stream_t stream);
/* Producers with the NEXT layer's quint8 quantiser fused in (converted PyTorchINT8 model; bit-identical to producer +
 * mv_quant_affine_i8): LayerNorm (vit.py:37,41) and the exact-fp32 attention core (vit.py:92-97, quant_out) writing int8
 * codes q - 128 [rows, dim] / [B, N, H*64] directly.  With MV_EPI_GELU_Q8 above they remove every fp32 activation tensor
 * between an int8 model's Linear layers except the q/k/v projections and the residual stream. */
int mv_layernorm_fwd_q8(const float* x, long ldx, const float* gamma, const float* beta, void* codes, int rows, int dim,
                        float eps, float scale, int zero_point, mv_stream_t stream);
int mv_attention_fwd_f32_q8(const float* qkv, void* codes, int B, int N, int H, float scale, float q_scale, int q_zero_point,
                            mv_stream_t stream);
/* The exact-fp32 attention core (Attention.forward vit.py:87-96) for any 1 <= N <= 8192 (384^2 fine-tuning: 577 tokens, 512^2
 * segmentation: 1 025): key-tiled kernels on the same f32-input matrix cores, so no [N, N] tensor exists in either direction.
 * Layouts, arithmetic and outputs as mv_attention_fwd_f32 (lse == NULL: evaluation), mv_attention_fwd_f32_lse, mv_attention_fwd_f32_q8
 * (codes bit-identical to mv_attention_fwd_long_f32 + mv_quant_affine_i8) and mv_attention_bwd_f32; the online softmax sums in
 * another order.  delta_ws: a caller-provided fp32 workspace of B * H * N floats (rowsum(dout * out)), required.  Deterministic: no
 * atomics, every output element has one owner.  MV_ERR_UNSUPPORTED for N > 8192 or a zero point outside 0..255.
 * ops.attention_fwd_f32 / _f32_lse / _f32_q8 / attention_bwd_f32_fused take these for N > 272 and the kernels above otherwise. */
int mv_attention_fwd_long_f32(const float* qkv, float* out, float* lse, int B, int N, int H, float scale, mv_stream_t stream);
int mv_attention_fwd_long_f32_q8(const float* qkv, void* codes, int B, int N, int H, float scale, float q_scale,
                                 int q_zero_point, mv_stream_t stream);
int mv_attention_bwd_long_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* delta_ws,
                              float* dqkv, int B, int N, int H, float scale, mv_stream_t stream);
/* running min/max observer: minmax[0] = min(minmax[0], min x), minmax[1] = max(minmax[1], max x);
 * minmax points at FOUR floats: [2..3] are scratch for the reduction */
int mv_minmax(const float* x, long n, float* minmax, mv_stream_t stream);

/* ---- loss: nn.CrossEntropyLoss() mean reduction -- classification/train.py:170,250; segmentation/train.py:188,261 ----
 * logits fp32 viewed as [outer, C, inner] (classification: inner = 1; segmentation: outer = B, inner = H*W);
 * labels int64 [outer*inner]: torch semantics -- ignore_index -100 gives no loss / gradient and is left out of the mean;
 *   any other label outside [0, C) is never dereferenced and turns the loss into NaN (torch device-asserts there);
 * loss_sum: fp32 [4], zeroed by this call: [0] = sum of per-sample losses / count (NaN when count = 0, as torch),
 *   [1] = count of non-ignored labels, [2] = number of out-of-range labels, [3] unused;
 * dlogits (optional, dl_dtype, same layout, row length ld_dl >= C when inner == 1 with zeroed padding)
 *   = (softmax - onehot) * grad_scale / count, zero rows for ignored labels.  argmax (optional int64 [outer*inner]). */
int mv_cross_entropy(const float* logits, const int64_t* labels, float* loss_sum, void* dlogits, int dl_dtype,
                     int ld_dl, int64_t* argmax, long outer, int C, long inner, float grad_scale,
                     mv_stream_t stream);

/* ---- soft-target loss and batch mixing (csrc/mixup.hip).  The reference has neither: these replace what a timm-style recipe
 * composes from torch ops -- timm.data.Mixup (batch mode: mixup_target's one_hot / flip / blend, and the image blend or box copy
 * of Mixup._mix_batch) and timm.loss.SoftTargetCrossEntropy / LabelSmoothingCrossEntropy.  Sample i of a batch of B is paired
 * with j = B - 1 - i (x.flip(0)); lam and the box are HOST scalars, so nothing is copied back and nothing synchronises. ----
 * mv_cross_entropy_soft: logits fp32 [B, C] dense, labels int64 [B].  Target t_i = lam * s(y_i) + (1 - lam) * s(y_j) with
 *   s(y) = eps / C everywhere plus (1 - eps) at class y; it is never materialised.  pair_flip = 0: no partner (y_j = y_i),
 *   requires lam == 1.  lam = 1, eps = 0 is the plain mean cross entropy; eps > 0 alone is cross_entropy(label_smoothing=eps).
 *   sample_loss: caller-provided fp32 [B] workspace, left holding  lse_i - (1-eps) * (lam * z[i,y_i] + (1-lam) * z[i,y_j])
 *     - (eps/C) * sum_c z[i,c];  loss: fp32 [1] = their mean, by one fixed-order reduction in a second one-wave launch -- no
 *   floating-point atomics, so loss and gradient are bitwise reproducible run to run.
 *   dlogits (optional, fp32 [B, C]) = (softmax(z_i) - t_i) * grad_scale / B.  argmax (optional, int64 [B]): first index wins.
 *   A label outside [0, C), the sample's own or its partner's, is never used as an index: that sample's loss and the mean are
 *   NaN and its dlogits row is zero.  No ignore_index (classification only).  One wave per sample: any C >= 2.
 *   MV_ERR_SHAPE: B < 0 or C < 2; MV_ERR_ALIGN: a null logits / labels / loss / sample_loss; MV_ERR_UNSUPPORTED: eps outside
 *   [0, 1), lam outside [0, 1], or pair_flip == 0 with lam != 1.  B == 0: nothing is launched and no pointer is looked at, MV_OK.
 * mv_mix_batch: x = dense [B, Ch, H, W] of `elem` (MV_F32 | MV_BF16, else MV_ERR_UNSUPPORTED), 16-byte aligned, mixed IN PLACE:
 *   each of the B / 2 pairs is visited once and a thread owns the same element of both samples (reads both, then writes both).
 *   For odd B the middle sample is its own partner and is not touched.
 *   mode 0, Mixup: x_i' = lam * x_i + (1 - lam) * x_j and x_j' = lam * x_j + (1 - lam) * x_i in fp32, one rounding to `elem`;
 *     16-byte accesses over the flat Ch * H * W extent wherever both samples sit at the same offset from a 16-byte boundary,
 *     single elements elsewhere.  lam == 1 launches nothing.  The box is ignored.
 *   mode 1, CutMix: rows [y0, y1) x columns [x0, x1) of every channel are swapped between x_i and x_j bit for bit; only the box
 *     is read or written (the launch covers its rows alone).  An empty box launches nothing.  lam is ignored: the caller sets
 *     lam = 1 - box_area / (H * W) for the loss.
 *   MV_ERR_SHAPE: a dimension <= 0, B < 0, or not 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W (mode 1); MV_ERR_ALIGN: x null or not
 *   16-byte aligned; MV_ERR_UNSUPPORTED: another mode, lam outside [0, 1] (mode 0), more than 65 535 pairs or Ch*H*W >= 2^31. */
int mv_cross_entropy_soft(const float* logits, const int64_t* labels, float* loss, float* sample_loss, float* dlogits,
                          int64_t* argmax, int B, int C, float lam, float eps, int pair_flip, float grad_scale,
                          mv_stream_t stream);
int mv_mix_batch(void* x, int elem, int B, int Ch, int H, int W, int mode, float lam, int y0, int y1, int x0, int x1,
                 mv_stream_t stream);

/* ---- DeiT distillation loss (csrc/distill.hip): DistillWrapper.forward, models/distill.py:142-151 --
 *   F.cross_entropy(student, labels) * alpha + F.kl_div(log_softmax(distill / T), softmax(teacher / T), "batchmean") * T^2 * (1 - alpha)
 * -- with both gradients and the student's arg-max from one launch plus a one-wave fixed-order mean.
 * student (class logits), distill (distillation-head logits), teacher: fp32 [B, C] dense; labels int64 [B].  Per sample:
 *   CE_i = the per-sample value of mv_cross_entropy_soft on the student row (same lam, eps, pair_flip; lam = 1, eps = 0 is the
 *          plain cross entropy), term for term;
 *   mode MV_DISTILL_SOFT (0):  KD_i = T^2 * sum_c p_c (log p_c - log q_c), p = softmax(teacher_i / T), q = softmax(distill_i / T);
 *          a class with p_c == 0 adds 0 (torch's kl_div);
 *   mode MV_DISTILL_HARD (1):  KD_i = lse(distill_i) - distill_i[argmax_c teacher_i], first index wins, T unused (DeiT's
 *          hard-label distillation; an extension, the reference has the soft form only).
 * loss: fp32 [3] = (alpha * mean CE + (1 - alpha) * mean KD, mean CE, mean KD).  sample_loss: caller-provided fp32 [2 * B]
 *   workspace, left holding CE_i in [0, B) and KD_i in [B, 2B); the means are one fixed-order reduction in a second one-wave
 *   launch -- no floating-point atomics and no memset, so loss and gradients are bitwise reproducible run to run.  Nothing is read
 *   back: the call can be captured in a graph.
 * dstudent (optional, fp32 [B, C]) = alpha * (softmax(student_i) - target_i) * grad_scale / B;
 * ddistill (optional, fp32 [B, C]) = (1 - alpha) * T * (q - p) * grad_scale / B (soft),
 *                                    (1 - alpha) * (softmax(distill_i) - onehot(argmax teacher_i)) * grad_scale / B (hard);
 *   a gradient whose weight is zero (alpha == 0, alpha == 1) is written as +0 throughout.  The teacher gets no gradient and is only read.
 * argmax (optional, int64 [B]): arg-max of the student row, first index wins.
 * A label outside [0, C), the sample's own or its partner's, is never used as an index: CE_i, the CE mean and the total are NaN
 *   and its dstudent row is zero; KD_i and its ddistill row do not depend on the label.  One wave per sample: any C >= 2.
 * MV_ERR_SHAPE: B < 0 or C < 2; MV_ERR_UNSUPPORTED: another mode, T <= 0 (or not finite), alpha outside [0, 1], eps outside
 *   [0, 1), lam outside [0, 1], or pair_flip == 0 with lam != 1; MV_ERR_ALIGN: a null student / distill / teacher / labels / loss
 *   / sample_loss.  B == 0: nothing is launched and no pointer is looked at, MV_OK. */
#define MV_DISTILL_SOFT 0
#define MV_DISTILL_HARD 1
int mv_distill_loss(const float* student, const float* distill, const float* teacher, const int64_t* labels, float* loss,
                    float* sample_loss, float* dstudent, float* ddistill, int64_t* argmax, int B, int C, int mode, float T,
                    float alpha, float lam, float eps, int pair_flip, float grad_scale, mv_stream_t stream);

/* ---- bilinear upsample (align_corners=False): nn.Upsample(size, 'bilinear') vit.py:355,371 ----
 * small[b, c, y, x] is read at  small + b*sb + c*sc + (y*w + x)*sp  (so the [B, h*w, C] output of the decoder GEMM is
 * consumed in place: the reference's transpose/view, vit.py:367-369, costs nothing); big: fp32 [B, C, H, W] dense.
 * backward is the exact adjoint in gather form (deterministic). */
int mv_upsample_bilinear_fwd(const float* small, long sb, long sc, long sp, float* big, int B, int C, int h, int w,
                             int H, int W, mv_stream_t stream);
int mv_upsample_bilinear_bwd(const float* dbig, float* dsmall, long sb, long sc, long sp, int B, int C, int h, int w,
                             int H, int W, mv_stream_t stream);

/* ---- fused segmentation tail: CrossEntropyLoss()(Upsample(size=(H,W),'bilinear')(small), labels) ----
 * replaces vit.py:355,371 (SegmentationDecoder.upsample) + segmentation/train.py:188,261-265 (criterion, argmax, accuracy)
 * in one pass that never materialises the [B, C, H, W] logits.
 * small: fp32 [B, h*w, C] (the decoder GEMM output, consumed in place); labels: int64 [B, H, W] in [0, C), or -100
 *      (ignore_index: no loss, no gradient, not counted in the mean); other out-of-range labels make the loss NaN.
 * fwd: lse fp32 [B,H,W] (log-sum-exp per pixel, kept for the backward), pred uint8 [B,H,W] (first-index arg-max),
 *      partials fp32 [4 * mv_seg_ce_partials(B,H,W)] scratch, stats fp32 [4]: [0] = mean loss over the counted labels,
 *      [1] = pixel accuracy over all pixels, [2] = counted labels, [3] = out-of-range labels.
 * bwd: stats = the forward's (its count is the mean's denominator; NULL: every pixel counts);
 *      dsmall (ds_dtype, [B*h*w, ld_ds], columns [C, ld_ds) zeroed) = d(mean loss)/d(small) * grad_scale; gather form,
 *      deterministic.  MV_ERR_UNSUPPORTED when C > 32 (bwd) or the per-image map does not fit 64 KB of LDS: compose
 *      mv_upsample_bilinear_* with mv_cross_entropy instead. */
long mv_seg_ce_partials(int B, int H, int W);
int mv_seg_ce_fwd(const float* small, const int64_t* labels, float* lse, uint8_t* pred, float* partials, float* stats,
                  int B, int C, int h, int w, int H, int W, mv_stream_t stream);
int mv_seg_ce_bwd(const float* small, const int64_t* labels, const float* lse, const float* stats, void* dsmall,
                  int ds_dtype, int ld_ds, float grad_scale, int B, int C, int h, int w, int H, int W, mv_stream_t stream);

/* ---- fused segmentation tail with a training recipe (csrc/seg_loss.hip): class weights, label smoothing, soft Dice ----
 * An extension: the reference trains segmentation on the plain mean cross entropy only (segmentation/train.py:188), which stays
 * with mv_seg_ce_* above, untouched.  With z = the bilinearly upsampled logits (the expressions of mv_seg_ce_*), p = softmax(z),
 * y the label, w_c = class_weight[c] (NULL: ones; a DEVICE array, >= 0), eps = label_smoothing, lam = dice_weight, s = dice_smooth,
 * "valid" = 0 <= y < C (y == -100 is ignored: no loss, no gradient, not counted; any other label outside [0, C) makes the loss NaN,
 * is never used as an index and gives no gradient):
 *   CE   = [(1-eps) sum_valid w_y (lse - z_y) + (eps/C) sum_valid sum_c w_c (lse - z_c)] / W,   W = sum_valid w_y
 *          (= torch.nn.functional.cross_entropy(z, y, weight=w, label_smoothing=eps); NaN when W == 0)
 *   Dice = 1 - (1/C) sum_c (2 I_c + s) / (P_c + N_c + s),  I_c = sum_valid p_c [y=c], P_c = sum_valid p_c, N_c = sum_valid [y=c]
 *          (over the whole batch; 0 when lam == 0)
 *   loss = CE + lam Dice
 * fwd: small fp32 [B, h*w, C], labels int64 [B, H, W]; lse fp32 [B,H,W] and pred uint8 [B,H,W] are bitwise those of mv_seg_ce_fwd;
 *      partials fp32 [mv_seg_loss_partials(B,C,H,W)] scratch (0 for an empty batch); stats fp32 [8]: [0] loss, [1] pixel accuracy
 *      over all pixels, [2] counted labels, [3] out-of-range labels, [4] CE, [5] Dice, [6] W, [7] 0; coef fp32 [2*C] = (a_c | b_c),
 *      a_c = -(2/C)/U_c, b_c = (1/C)(2 I_c + s)/U_c^2, U_c = P_c + N_c + s (zeros when lam == 0); areas int64 [3*C] or NULL =
 *      (intersect_c | pred_c | label_c) with the semantics of utils/miou.intersect_and_union: pred_c over all pixels, intersect_c
 *      where pred == label == c, labels outside [0, C) dropped.  Bitwise reproducible: every float sum has a fixed order (no float
 *      atomics), counts are integers throughout (int64 totals).  Never synchronises, no memset: graph-capture safe.
 *      B == 0: a kernel clears stats and areas, MV_OK.
 * bwd: lse, stats, coef = the forward's (coef may be NULL when dice_weight == 0); dsmall (element type ds_elem = MV_F32 | MV_BF16,
 *      [B*h*w, ld_ds], columns [C, ld_ds) zeroed) = d(loss)/d(small) * grad_scale, gather form, deterministic; per valid pixel
 *        dz_c = [p_c ((1-eps) w_y + (eps/C) sum_k w_k) - (1-eps) w_y [y=c] - (eps/C) w_c] / W + lam p_c (g_c - sum_k p_k g_k),
 *        g_c = a_c [y=c] + b_c;   all zero when W == 0.
 * MV_ERR_SHAPE: a non-positive dimension, B < 0, B > 65535, ld_ds < C.  MV_ERR_UNSUPPORTED: C > 32; the per-image map (plus, in
 * bwd, W*C column sums) beyond 64 KB of LDS; label_smoothing outside [0, 1); dice_weight < 0; dice_weight > 0 with
 * dice_smooth <= 0; ds_elem neither MV_F32 nor MV_BF16.  All answered before any launch. */
long mv_seg_loss_partials(int B, int C, int H, int W);
int mv_seg_loss_fwd(const float* small, const int64_t* labels, const float* class_weight, float label_smoothing,
                    float dice_weight, float dice_smooth, float* lse, uint8_t* pred, float* partials, float* stats, float* coef,
                    int64_t* areas, int B, int C, int h, int w, int H, int W, mv_stream_t stream);
int mv_seg_loss_bwd(const float* small, const int64_t* labels, const float* class_weight, float label_smoothing,
                    float dice_weight, const float* lse, const float* stats, const float* coef, void* dsmall, int ds_elem,
                    int ld_ds, float grad_scale, int B, int C, int h, int w, int H, int W, mv_stream_t stream);

/* ---- YOLOS detection tail (csrc/detection.hip).  Everything is fp32 in every precision; Q = num_det_tokens queries per image,
 * C1 = num_classes + 1 (the last class is "no object"), boxes are (cx, cy, w, h) in [0, 1]. ----
 * decoder: vit.py:376-396 DetectionDecoder.forward -- x[:, -Q:, :] -> class_embed, bbox_embed + sigmoid -- in one pass over the
 * gathered rows.  x: [B, T, D] (only its last Q rows per image are read); logits [B, Q, C1]; boxes [B, Q, 4] (after the sigmoid).
 * bwd: dlogits / dboxes (either may be NULL = zero) -> dx (NULL, or [B, T, D] whose last Q rows per image are WRITTEN, the caller
 * zero-fills the rest), dw_cls [C1, D], db_cls [C1], dw_box [4, D], db_box [4]; the sigmoid derivative is applied in-kernel from
 * the saved boxes.  Deterministic: row slabs into the workspace, then a fixed-order sum. */
int mv_det_heads_fwd(const float* x, const float* w_cls, const float* b_cls, const float* w_box, const float* b_box,
                     float* logits, float* boxes, int B, int T, int Q, int D, int C1, mv_stream_t stream);
size_t mv_det_heads_bwd_workspace_bytes(int B, int Q, int D, int C1);
int mv_det_heads_bwd(const float* x, const float* w_cls, const float* w_box, const float* boxes, const float* dlogits,
                     const float* dboxes, float* dx, float* dw_cls, float* db_cls, float* dw_box, float* db_box,
                     void* workspace, size_t workspace_bytes, int B, int T, int Q, int D, int C1, mv_stream_t stream);
/* sequence assembly YOLOS intends (vit.py:285-302 with its "detection" branch taken, which the reference never does):
 * out [B, T0 + Q, D] = cat(x [B, T0, D], det [Q, D] + pos [Q, D]).  bwd: dx [B, T0, D] = dout[:, :T0], ddet = dpos [Q, D] = the
 * sum over the batch of dout[:, T0:], in batch order (no float atomics). */
int mv_det_append_fwd(const float* x, const float* det, const float* pos, float* out, int B, int T0, int Q, int D,
                      mv_stream_t stream);
int mv_det_append_bwd(const float* dout, float* dx, float* ddet, float* dpos, int B, int T0, int Q, int D,
                      mv_stream_t stream);
/* matching cost, matcher.py:58-82: only the per-image blocks of the reference's [B*Q, sum T] matrix.  labels int64 [sum T],
 * tboxes [sum T, 4], toff int32 [B + 1] (prefix sums of the target counts).  out: packed fp32, the [Q, T_b] block of image b
 * (row-major) starts at Q * toff[b]:  cost_bbox * L1 - cost_class * softmax(logits)[label] - cost_giou * GIoU
 * (torchvision's generalized_box_iou on the xyxy boxes, no epsilon).  A label outside [0, C1) gives NaN. */
int mv_det_cost(const float* logits, const float* boxes, const int64_t* labels, const float* tboxes, const int32_t* toff,
                float* out, float cost_class, float cost_bbox, float cost_giou, int B, int Q, int C1, mv_stream_t stream);
/* the assignment itself, matcher.py:84-86 (scipy.optimize.linear_sum_assignment per image), on the device: one wave per image
 * solves the rectangular minimum-cost assignment of its [Q, T_b] block of mv_det_cost's output exactly (shortest augmenting
 * paths, Crouse 2016, fp64 duals over the fp32 costs; +inf = a forbidden pair), pairing min(Q, T_b) queries and targets.
 * max_t: the largest T_b (host-known); Q and max_t at most 1024 (MV_ERR_UNSUPPORTED above).  match int32 [B * Q], every element
 * written: the flat target index toff[b] + t of query q, or -1 -- what mv_det_assign reads.  status int32 [B]: 0 solved (also
 * T_b = 0), 1 the block holds a NaN or -inf (or T_b lies outside [0, max_t]), 2 infeasible (every complete assignment needs a
 * +inf entry); for status != 0 every match entry of that image is -1.  Deterministic: ties go to the smaller path cost, then an
 * unassigned column, then the lower index, so the pairs equal scipy's wherever the optimum is unique. */
int mv_det_match(const float* cost, const int32_t* toff, int32_t* match, int32_t* status, int B, int Q, int max_t,
                 mv_stream_t stream);
/* detector.py:48-52,82-84: per-query targets from the matching.  match int32 [n]: flat target index of query i or -1 ->
 * tgt_class int64 [n] (no_object where unmatched), tgt_box [n, 4] (zeros where unmatched). */
int mv_det_assign(const int32_t* match, const int64_t* labels, const float* tboxes, int64_t* tgt_class, float* tgt_box, long n,
                  long ntargets, int no_object, mv_stream_t stream);
/* SetCriterion, detector.py:41-98, one launch each way.  weight [C1] (empty_weight), tcount int32 [B] (targets per image),
 * inv_num_boxes = 1 / num_boxes (detector.py:134-138).  fwd: lse [B*Q] (kept for the backward), stats fp32 [8]:
 * [0] loss_ce = sum w[t] nll / sum w[t], [1] loss_bbox = sum |d| / num_boxes, [2] loss_giou = sum (1 - GIoU) / num_boxes over the
 * matched queries (tgt_class != C1 - 1), [3] class_error = 100 - top-1 accuracy over the matched queries (100 when none),
 * [4] cardinality_error, [5] sum w[t], [6] matched queries, [7] target classes outside [0, C1) (then [0] is NaN).
 * bwd: g_ce / g_bbox / g_giou: device scalars (NULL = 0), the incoming gradients of stats[0..2] -> dlogits [B, Q, C1], dboxes
 * [B, Q, 4] (zero rows for unmatched queries), every element written once. */
int mv_det_loss_fwd(const float* logits, const float* boxes, const int64_t* tgt_class, const float* tgt_box, const float* weight,
                    const int32_t* tcount, float* lse, float* stats, float inv_num_boxes, int B, int Q, int C1,
                    mv_stream_t stream);
int mv_det_loss_bwd(const float* logits, const float* boxes, const int64_t* tgt_class, const float* tgt_box, const float* weight,
                    const float* lse, const float* stats, const float* g_ce, const float* g_bbox, const float* g_giou,
                    float* dlogits, float* dboxes, float inv_num_boxes, int B, int Q, int C1, mv_stream_t stream);
/* PostProcess.forward, detector.py:159-176: scores [B, Q] / labels int64 [B, Q] = max / first arg-max of the softmax over the real
 * classes, out_boxes [B, Q, 4] = xyxy * (w, h, w, h); sizes fp32 [B, 2] = (height, width). */
int mv_det_postprocess(const float* logits, const float* boxes, const float* sizes, float* scores, int64_t* labels,
                       float* out_boxes, int B, int Q, int C1, mv_stream_t stream);

/* ---- image batch preparation: Normalize(ToTensor(hflip?(resize(crop(img, box), size, BILINEAR)))) ----
 * replaces the per-image torchvision/Pillow pipeline of the DataLoader worker (datasets/resisc45.py:40-69,
 * datasets/dlrsd.py:39-66, transforms/segmentation.py) on decoded uint8 frames, bit-exact to Pillow's 8-bit resampler.
 * src: uint8 [B][Hs][Ws][3] (images img_stride bytes apart).  Per image and axis the host supplies Pillow's
 * precompute_coeffs tables with crop offset / CenterCrop window folded in: bounds bh/bv int32 [B, out, 2] = (first
 * source index, tap count <= ks) and 22-bit fixed-point coefficients kh/kv int32 [B, out, ks].  flip: uint8 [B].
 * out: fp32 [B, 3, out_h, out_w] = ((pixel / 255) - mean[c]) / std[c]  (mean 0, std 1: plain ToTensor). */
int mv_image_prepare(const uint8_t* src, long img_stride, int Hs, int Ws, const int32_t* kh, const int32_t* bh,
                     const int32_t* kv, const int32_t* bv, int ks, const uint8_t* flip, float mean0, float mean1,
                     float mean2, float std0, float std1, float std2, float* out, int B, int out_h, int out_w,
                     mv_stream_t stream);
/* segmentation masks: Image.resize(NEAREST) of the crop as a gather through per-axis source index tables yi [B, out_h],
 * xi [B, out_w] (Pillow's ImagingScaleAffine indices, crop offset folded in); out int64 [B, out_h, out_w] = src + add
 * (DLRSD labels are PNG value - 1, datasets/dlrsd.py:80). */
int mv_mask_prepare(const uint8_t* src, long img_stride, int Hs, int Ws, const int32_t* yi, const int32_t* xi,
                    const uint8_t* flip, int add, int64_t* out, int B, int out_h, int out_w, mv_stream_t stream);
/* stage one of a Resize -> RandomResizedCrop chain (segmentation/data_configs/data_config.json transform_ops_train, built
 * by datasets/dlrsd.py:39-66): the same resampling with the result kept as uint8 -- out [B, out_h, out_w, 3] (frames) /
 * [B, out_h, out_w] (masks, NEAREST) -- because every Pillow resize rounds to uint8, so the second resize must start
 * from that image.  Tables as for mv_image_prepare / mv_mask_prepare; no flip, no normalisation. */
int mv_image_resize_u8(const uint8_t* src, long img_stride, int Hs, int Ws, const int32_t* kh, const int32_t* bh,
                       const int32_t* kv, const int32_t* bv, int ks, uint8_t* out, int B, int out_h, int out_w,
                       mv_stream_t stream);
int mv_mask_resize_u8(const uint8_t* src, long img_stride, int Hs, int Ws, const int32_t* yi, const int32_t* xi, uint8_t* out,
                      int B, int out_h, int out_w, mv_stream_t stream);
/* ragged batches (detection/train.py: transforms/detection.py from_config + nested_tensor_from_tensor_list): sample b has its own
 * output extent ext[b] = (oh_b, ow_b) <= (out_h, out_w), int32 [B, 2], inside one padded batch.  Tables as above but padded to
 * out_w / out_h rows per sample (rows past the extent are not read); a horizontal flip is folded into the horizontal tables by
 * the host (taps reversed), so there is no flip argument.  out fp32 [B, 3, out_h, out_w]: the normalised image on the extent and
 * exactly 0.0 elsewhere (the reference pads after Normalize); pad_mask uint8 (bool) [B, out_h, out_w]: 0 on the extent, 1 on the
 * padding.  Every element of both is written by the one launch.  _u8: the intermediate uint8 [B, out_h, out_w, 3] frame of a
 * two-resampling chain (PreRandomResize -> RandomSizeCrop -> PostRandomResize), zeros outside the extent. */
int mv_image_prepare_ragged(const uint8_t* src, long img_stride, int Hs, int Ws, const int32_t* kh, const int32_t* bh,
                            const int32_t* kv, const int32_t* bv, int ks, const int32_t* ext, float mean0, float mean1,
                            float mean2, float std0, float std1, float std2, float* out, uint8_t* pad_mask, int B, int out_h,
                            int out_w, mv_stream_t stream);
int mv_image_resize_u8_ragged(const uint8_t* src, long img_stride, int Hs, int Ws, const int32_t* kh, const int32_t* bh,
                              const int32_t* kv, const int32_t* bv, int ks, const int32_t* ext, uint8_t* out, int B, int out_h,
                              int out_w, mv_stream_t stream);

/* ---- optimizer: AdamW step (timm create_optimizer 'adamw' -> torch.optim.AdamW), classification/train.py:161-166,274-277 ----
 * flat fp32 arrays of n elements; decoupled weight decay; bias corrections passed in (host computes from step) */
int mv_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
             float weight_decay, float bias_corr1, float bias_corr2, float grad_scale, const float* clip_coef,
             mv_stream_t stream);
/* the same step with the scalars that change from step to step read from DEVICE memory: hyper = fp32 [3] = (lr, bias_corr1,
 * bias_corr2).  A launch captured in a HIP graph (the whole training step of classification/train.py:239-279 replayed as one
 * graph) then stays valid while the learning-rate schedule and the step count advance: the host rewrites three floats. */
int mv_adamw_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                 float weight_decay, float grad_scale, const float* clip_coef, mv_stream_t stream);
/* the same step over a WHOLE parameter arena in one launch, with a learning-rate scale and a weight decay per tensor and an
 * optional weight EMA (an extension: layer-wise learning-rate decay, a no_weight_decay list and a model EMA, as timm's
 * create_optimizer(layer_decay=...) / ModelEmaV2 give the fine-tuning recipes; the reference has none of them).
 * Work list, cut on the host once and kept on the device: item i covers elements [item_off[i], item_off[i] + item_len[i]) of
 * p / g / m / v (and ema), never crosses a tensor, has 1 <= item_len[i] <= 4096, starts on a multiple of 8 elements (32 bytes:
 * a tensor's arena offset plus a multiple of 4096) and belongs to segment item_seg[i] in [0, n_seg).  A segment is a distinct
 * pair (lr_scale, weight_decay): seg_lr_scale[n_seg], seg_wd[n_seg], device fp32.  Workgroups stride over the items; within an
 * item float4 accesses over item_len & ~3 elements and scalar ones for the rest.  Per element the arithmetic of mv_adamw with
 * lr * seg_lr_scale[seg] for lr and seg_wd[seg] for weight_decay: with every scale 1 the same bits as mv_adamw writes over a
 * region whose length is a multiple of 4 (every region of a parameter arena).
 * (lr, bias_corr1, bias_corr2) come from the arguments, or from the device fp32 [3] hyper when that is non-null (mv_adamw_dev's
 * form, what a captured launch needs); grad_scale and the device scalar clip_coef (may be null) as in mv_adamw.
 * ema non-null: also ema[i] = ema_decay * ema[i] + (1 - ema_decay) * p_new[i], in the same pass.
 * Elements in no item (the alignment gaps between tensors) are neither read nor written.  No atomics, every element has one
 * owner: bitwise reproducible.  The items are trusted (a segment index or an extent outside the arrays is not detected).
 * Checks, in this order and before any launch: n_items < 0 or n_seg <= 0 -> MV_ERR_SHAPE; a beta outside [0, 1), or ema non-null
 * with ema_decay outside [0, 1) or NaN -> MV_ERR_UNSUPPORTED; n_items == 0 -> MV_OK, nothing launched; p / g / m / v null, any
 * of them or ema not 16-byte aligned, or a null item or segment table -> MV_ERR_ALIGN. */
int mv_adamw_table(float* p, const float* g, float* m, float* v, float* ema, const int64_t* item_off, const int32_t* item_len,
                   const int32_t* item_seg, long n_items, const float* seg_lr_scale, const float* seg_wd, int n_seg,
                   const float* hyper, float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                   float grad_scale, const float* clip_coef, float ema_decay, mv_stream_t stream);
/* ---- optimizer family: timm create_optimizer 'sgd' / 'momentum' (-> torch.optim.SGD, nesterov on / off) and 'lamb' (-> timm's
 * Lamb) on the work list of mv_adamw_table (an extension: every reference train_config says "adamw", classification/train.py:161-166).
 * Items, segments, hyper, grad_scale, clip_coef and ema / ema_decay as in mv_adamw_table; elements in no item are neither read nor
 * written; no atomics, bitwise reproducible.
 * mv_sgd_table, ONE launch.  Per element, gr = g * grad_scale (* clip_coef[0]), wd = seg_wd[seg] (torch.optim.SGD, dampening 0):
 *   d = gr + wd * p;  buf = momentum * buf + d;  d = nesterov ? d + momentum * buf : buf;  p -= lr * seg_lr_scale[seg] * d
 * momentum == 0: d stays gr + wd * p and buf is neither read nor written (it may be null).  A zero buf makes the first step
 * buf = d, as torch's first step does.  Of hyper only hyper[0], the rate, is read.
 * Checks, in this order and before any launch: n_items < 0 or n_seg <= 0 -> MV_ERR_SHAPE; momentum outside [0, 1) or NaN, nesterov
 * with momentum == 0, or ema non-null with ema_decay outside [0, 1) -> MV_ERR_UNSUPPORTED; n_items == 0 -> MV_OK, nothing launched;
 * p / g null, buf null with momentum != 0, any of them or ema not 16-byte aligned, or a null table -> MV_ERR_ALIGN. */
int mv_sgd_table(float* p, const float* g, float* buf, float* ema, const int64_t* item_off, const int32_t* item_len,
                 const int32_t* item_seg, long n_items, const float* seg_lr_scale, const float* seg_wd, int n_seg,
                 const float* hyper, float lr, float momentum, int nesterov, float grad_scale, const float* clip_coef,
                 float ema_decay, mv_stream_t stream);
/* mv_lamb_table, TWO launches on the stream.  timm's Lamb with bias correction on, always_adapt off and no trust clip (its global
 * gradient clip is the caller's mv_grad_norm_clip, handed in as clip_coef):
 *   m = beta1 * m + (1 - beta1) * gr;  v = beta2 * v + (1 - beta2) * gr * gr
 *   u = (m / bias_corr1) / (sqrt(v) / sqrt(bias_corr2) + eps) + wd * p
 *   trust = (wd != 0 && ||p|| > 0 && ||u|| > 0) ? ||p|| / ||u|| : 1          (norms over the element's TENSOR)
 *   p -= lr * seg_lr_scale[seg] * trust * u
 * Launch 1 writes m and v and leaves (sum p^2, sum u^2) of every item, two doubles, in workspace.  Launch 2 runs per item again:
 * its workgroup adds the pairs of all items of the item's tensor in a fixed order (in double), forms trust, recomputes u from the new
 * m, v and the unchanged p, and writes p (and ema).  No atomics, no memset, no word passed between workgroups of one launch: every
 * item of a tensor sees the same bits of trust, and a tensor's result depends neither on the grid nor on the rest of the arena.
 * Two more device tables say which items form a tensor: item_tensor[n_items], the tensor of each item, in [0, n_tensors), and
 * tensor_range[2 * n_tensors] = (first item, item count) of each tensor; a tensor's items are consecutive.  The tables are trusted.
 * workspace: mv_lamb_workspace_bytes(n_items) bytes (16 per item), 16-byte aligned, owned by the caller and kept between calls (a
 * captured step replays on it); it needs no initialisation.
 * Checks, in this order and before any launch: n_items < 0, n_seg <= 0, n_tensors < 0 or n_tensors == 0 with items -> MV_ERR_SHAPE;
 * a beta outside [0, 1), or ema non-null with ema_decay outside [0, 1) -> MV_ERR_UNSUPPORTED; n_items == 0 -> MV_OK, nothing
 * launched; p / g / m / v null, any of them or ema not 16-byte aligned, a null table, or workspace null, misaligned or too small
 * -> MV_ERR_ALIGN. */
size_t mv_lamb_workspace_bytes(long n_items);
int mv_lamb_table(float* p, const float* g, float* m, float* v, float* ema, const int64_t* item_off, const int32_t* item_len,
                  const int32_t* item_seg, const int32_t* item_tensor, long n_items, const int32_t* tensor_range, int n_tensors,
                  const float* seg_lr_scale, const float* seg_wd, int n_seg, const float* hyper, float lr, float beta1, float beta2,
                  float eps, float bias_corr1, float bias_corr2, float grad_scale, const float* clip_coef, float ema_decay,
                  void* workspace, size_t workspace_bytes, mv_stream_t stream);
/* ---- gradient clipping: torch.nn.utils.clip_grad_norm_(vit.parameters(), clip_grad), classification/train.py:265-270 ----
 * over the flat gradient array g[n]: out[0] = total_norm = ||g * grad_scale||_2, out[1] = min(1, max_norm / (total_norm + 1e-6)).
 * out stays on the device; pass out + 1 as mv_adamw's clip_coef (it multiplies every gradient there: no extra pass).
 * workspace: mv_grad_norm_workspace_bytes() bytes, 16-byte aligned.  Deterministic (fixed summation order). */
size_t mv_grad_norm_workspace_bytes(void);
int mv_grad_norm_clip(const float* g, long n, float grad_scale, float max_norm, float* out, void* workspace,
                      size_t workspace_bytes, mv_stream_t stream);

/* ---- dropout: nn.Dropout(p) in training mode -- vit.py:50,52 (FeedForward), :75 (Attention.to_out), :311 (embedding) ----
 * y[i] = x[i] * keep_i / (1 - p), keep_i = (word (i & 3) of Philox4x32-10(counter = (i >> 2, offset), key = seed) >= p * 2^32).
 * The same call with (seed, offset) on the output gradient IS the backward: no mask is stored.  x == y allowed.
 * (The reference draws its mask from torch's generator: same distribution, different stream -- parity is statistical.) */
int mv_dropout(const void* x, void* y, int dtype, long n, float p, uint64_t seed, uint64_t offset, mv_stream_t stream);

/* ---- stochastic depth ("drop path": timm's DropPath, scale_by_keep=True): one factor per sample and residual branch ----
 * mv_drop_path_draw, ONE launch of one workgroup: table[r * B + b] = keep ? scale[r] : 0 for R branches and B samples, where
 * keep = (word (e & 3) of Philox4x32-10(counter = (e >> 2, step), key = seed) >= thr[r]), e = r * B + b: mv_dropout's mask of
 * R * B elements with offset = step.  state is a device uint64[2] = (seed, step), 16-byte aligned; after every read of it the
 * kernel stores step + 1, so the next call (or the next replay of a captured call) draws the next table with no host value
 * involved.  thr[R] = (uint32)(p_r * 2^32) and scale[R] = (float)(1 / (1 - p_r)) are the caller's, computed once in double.
 * R * B <= 2^24 (MV_ERR_SHAPE beyond); R * B == 0 launches nothing and leaves state alone. */
int mv_drop_path_draw(uint64_t* state, const uint32_t* thr, const float* scale, float* table, int R, int B, mv_stream_t stream);
/* In place on f, both fp32 [B, per_sample], c fp32 [B]: f[b, :] = fmaf(c[b], f[b, :], x[b, :]) where c[b] != 0, and exactly
 * x[b, :] where c[b] == 0 (f is then not read).  per_sample is arbitrary (a 16-byte vector that straddles samples takes one factor
 * per element); x and f 16-byte aligned. */
int mv_drop_path_add(const float* x, float* f, const float* c, int B, long per_sample, mv_stream_t stream);
/* out[b, :] = round_to_out_dtype(c[b] * (float)in[b, :]): one rounding of the fp32 product; in and out fp32 or bf16 (MV_F32 /
 * MV_BF16 as in_code / out_code, any pairing; MV_ERR_UNSUPPORTED otherwise), [B, per_sample], 16-byte aligned, not overlapping.  The backward of
 * mv_drop_path_add with respect to f (in = the output gradient), and its own backward. */
int mv_row_scale(const void* in, int in_code, void* out, int out_code, const float* c, int B, long per_sample,
                 mv_stream_t stream);

/* ---- Random Erasing (csrc/random_erase.hip): a restatement of timm's RandomErasing (timm.data.random_erasing, _erase) on the
 * project's Philox stream.  The reference has no call site: it never erases.  Same distribution as timm, different stream.
 * mv_random_erase_draw, ONE launch of one workgroup: reads state = device uint64[2] (seed, step), writes boxes = int32
 *   [B, max_count, 4] = (top, left, h, w) per erase (all four zero where nothing is erased) and used = device uint64[2], its own
 *   array: the (seed, step) of THIS draw, which the fill reads; then, after a barrier, stores step + 1 to state[1].  So the next
 *   call (or the next replay of a captured call) draws anew with no host value involved.  Per sample, in fp64: erased iff its
 *   sample word < thr (thr = (uint64)(probability * 2^32), so 2^32 erases every sample); count = min_count + umulhi(word,
 *   max_count - min_count + 1); per erase up to 10 attempts of  target = (min_area + u (max_area - min_area)) * H * W / count,
 *   ratio = exp(log_lo + u' (log_hi - log_lo)), h = rint(sqrt(target * ratio)), w = rint(sqrt(target / ratio)), accepted iff
 *   h < H and w < W, then top = umulhi(word, H - h + 1), left = umulhi(word, W - w + 1).  A box of zero extent is accepted and
 *   erases nothing; ten failures leave the slot empty.  The counter of every word: the header comment of random_erase.hip.
 *   area_ratio is a HOST array of four doubles (min_area, max_area, log_lo, log_hi), read before the launch: the C ABI passes no
 *   floating-point argument wider than float by value.
 *   MV_ERR_SHAPE: B < 0, H or W <= 0; MV_ERR_UNSUPPORTED: not 1 <= min_count <= max_count <= 8, thr > 2^32, not
 *   0 < min_area <= max_area <= 1, or not log_lo <= log_hi, both finite; MV_ERR_ALIGN: a null area_ratio, a null or not 16-byte aligned device array.
 *   B == 0 (with valid counts and thr) launches nothing, leaves state alone and looks at no pointer: MV_OK.
 * mv_random_erase_apply: fills x = dense [B, Ch, H, W] of `elem` (MV_F32 | MV_BF16) IN PLACE from boxes; write-only, x is never
 *   loaded.  mode 0 `const`: +0.0; mode 1 `rand`: one N(0,1) value per (sample, box, channel); mode 2 `pixel`: one N(0,1) value
 *   per element, a function of (used, flat element index) only.  Normals: Box-Muller in fp32.  Where boxes of one sample overlap,
 *   the LATER box wins (timm writes them in order) and no element is written twice; boxes are clipped to the image.  An empty
 *   slot costs one 16-byte read.  MV_ERR_SHAPE: B < 0 or a dimension <= 0; MV_ERR_UNSUPPORTED: another elem or mode, max_count
 *   outside 1..8, B*Ch*H*W >= 2^58 or B * max_count >= 2^31; MV_ERR_ALIGN: a null array or boxes not 16-byte aligned.  B == 0: MV_OK. */
int mv_random_erase_draw(uint64_t* state, int32_t* boxes, uint64_t* used, int B, int H, int W, uint64_t thr,
                         const double* area_ratio, int min_count, int max_count, mv_stream_t stream);
int mv_random_erase_apply(void* x, int elem, const int32_t* boxes, const uint64_t* used, int B, int Ch, int H, int W, int max_count,
                          int mode, mv_stream_t stream);

/* ---- RandAugment (csrc/randaug.hip, arithmetic in csrc/randaug_math.h): an extension -- the reference augments with crop and flip
 * only.  A restatement of timm's increasing op set (timm.data.auto_augment, `rand-m9-mstd0.5-inc1`), computed bit for bit as the
 * Pillow 12 calls of datasets/transforms.RandAugment compute it.  One SLOT of the whole batch per pair of calls: src / dst uint8
 * [B, H, W, 3]; ops int32 [B, num_ops] with ops[b, slot] = 0 (skipped: a copy) or 1..15 = AutoContrast, Equalize, Invert, Rotate,
 * Posterize, Solarize, SolarizeAdd, Color, Contrast, Brightness, Sharpness, ShearX, ShearY, TranslateX, TranslateY; par fp64
 * [B, num_ops, 8]: geometric ops (Rotate is an affine like the others, its matrix built by the host as Image.rotate builds it)
 * par[0..5] = the coefficients of Image.transform(AFFINE) and par[6] = 0 bilinear / 1 bicubic; enhance ops par[0] = the factor
 * (converted to float, as Image.blend does); Posterize / Solarize / SolarizeAdd par[0] = bits / threshold / addend.
 * mv_randaug_stats, one workgroup per sample: for AutoContrast and Equalize the 3 x 256 lookup table into tables uint8
 *   [B, 3, 256] (histograms by integer LDS atomics, table finished in the same launch; ImageOps.autocontrast in fp64, uncontracted;
 *   ImageOps.equalize in 64-bit integers), for Contrast mean[b] = (int)(sum of L / (H * W) + 0.5) with L = (19595 R + 38470 G +
 *   7471 B + 32768) >> 16.  A sample with any other op writes nothing.  No global atomic, no memset.
 * mv_randaug_apply: writes every byte of dst (src != dst; Sharpness and the geometric ops read neighbours of src).  Geometric: per
 *   output pixel xin = a0 (x + .5) + a1 (y + .5) + a2, yin likewise, fill colour where (xin, yin) is outside the image, else
 *   Geometry.c's bilinear / bicubic filter in fp64.  Enhance: (uint8)(d + f (s - d)) in fp32, clipped when f is outside [0, 1], with
 *   d = 0 (Brightness), L (Color), mean[b] (Contrast), ImageFilter.SMOOTH (Sharpness; border copied).  tables / mean are read
 *   only by the samples whose op mv_randaug_stats serves.
 * MV_ERR_SHAPE: B < 0 or > 65535, H or W <= 0, H * W * 3 >= 2^31, slot outside [0, num_ops); MV_ERR_UNSUPPORTED: a fill byte
 * outside 0..255; MV_ERR_ALIGN: a null array, src == dst, par not 8-byte aligned.  B == 0: MV_OK, nothing launched. */
int mv_randaug_stats(const uint8_t* src, const int32_t* ops, int num_ops, int slot, uint8_t* tables, int32_t* mean, int B, int H,
                     int W, mv_stream_t stream);
int mv_randaug_apply(const uint8_t* src, uint8_t* dst, const int32_t* ops, const double* par, int num_ops, int slot,
                     const uint8_t* tables, const int32_t* mean, int fill0, int fill1, int fill2, int B, int H, int W,
                     mv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MYRTLE_VISION_HIP_H */
