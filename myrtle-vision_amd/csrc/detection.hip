// YOLOS detection tail: everything after the last transformer block (reference: models/vit.py:376-396 DetectionDecoder,
// models/matcher.py:58-86 HungarianMatcher's cost matrix, models/detector.py:41-98 SetCriterion's three losses and two statistics,
// models/detector.py:159-176 PostProcess) and the sequence assembly YOLOS intends (vit.py:285-302, the branch the reference never
// takes).
//
// Every tensor here is small (100 queries, a few targets, 21-92 classes) and fp32 in every precision: the cost of this tail in
// torch is its launch count (dozens of kernels and several device <-> host round trips at batch 2), not its arithmetic.  So each
// step is ONE launch, shaped around queries:
//
//   heads fwd   : a workgroup stages 4 of the last Q rows of the sequence in LDS (the gather) and a wave per output column walks
//                 both heads' weight rows over them; the box head's sigmoid is the epilogue.  x is read once, not per head.
//   heads bwd   : dX = dY W (thread <-> feature, dY rows in LDS with the sigmoid derivative applied while staging);
//                 dW / db = dY^T X over row slabs into a workspace, then a fixed-order sum over the slabs (deterministic).
//   append      : [B, 1+P, D] + (det_tokens + pos_embedding_det) -> [B, 1+P+Q, D]; the backward copies the first 1+P rows and
//                 reduces the Q rows over the batch in batch order (no float atomics) into both parameters' gradients.
//   cost        : a wave per (image, query): softmax statistics once, then lanes over that image's targets only -- the
//                 [B*Q, sum T] matrix of the reference, of which only the per-image diagonal blocks are ever read, is not formed.
//   match       : a wave per image solves the assignment on its cost block (shortest augmenting paths, fp64 duals), so nothing
//                 between the transformer's output and the loss scalar waits for the host.
//   loss fwd    : one workgroup, threads over queries, fixed-order tree sums; the per-image cardinality counts are integer
//                 LDS atomics (exact, order-free).
//   loss bwd    : a thread per query writes its dlogits row and dbox from the three incoming gradient scalars.
//
// GIoU is torchvision.ops.generalized_box_iou's formula with no epsilon: degenerate boxes give inf/NaN exactly as there.
#include "mv_common.h"

namespace {

constexpr int DET_ROWS = 4;            // gathered rows per workgroup of the heads kernels
constexpr int DET_NMAX = 256;          // outputs of both heads together ((C + 1) + 4)
constexpr int DET_DW_NT = 4;           // output columns per workgroup of the dW kernel
constexpr int DET_DW_SLAB = 64;        // rows per slab of the dW kernel
constexpr int DET_DW_MAXSLABS = 64;
constexpr size_t DET_LDS_LIMIT = 64 * 1024;

struct DetBox { float x0, y0, x1, y1; };

// torchvision.ops.box_convert(in_fmt="cxcywh", out_fmt="xyxy")
__device__ __forceinline__ DetBox det_xyxy(const float* b) {
  return DetBox{b[0] - 0.5f * b[2], b[1] - 0.5f * b[3], b[0] + 0.5f * b[2], b[1] + 0.5f * b[3]};
}

// torchvision.ops.generalized_box_iou for one pair (no epsilon)
__device__ __forceinline__ float det_giou(const DetBox& p, const DetBox& t) {
  const float a1 = (p.x1 - p.x0) * (p.y1 - p.y0), a2 = (t.x1 - t.x0) * (t.y1 - t.y0);
  const float iw = fmaxf(fminf(p.x1, t.x1) - fmaxf(p.x0, t.x0), 0.f), ih = fmaxf(fminf(p.y1, t.y1) - fmaxf(p.y0, t.y0), 0.f);
  const float inter = iw * ih, uni = a1 + a2 - inter;
  const float ew = fmaxf(fmaxf(p.x1, t.x1) - fminf(p.x0, t.x0), 0.f), eh = fmaxf(fmaxf(p.y1, t.y1) - fminf(p.y0, t.y0), 0.f);
  const float ac = ew * eh;
  return inter / uni - (ac - uni) / ac;
}

// d GIoU / d (cx, cy, w, h) of the first box: the chain rule through max / min / clamp as autograd takes it away from ties
// (the selected operand gets the gradient; clamp passes it where the width is positive)
__device__ __forceinline__ void det_giou_grad(const DetBox& p, const DetBox& t, float g[4]) {
  const float pw = p.x1 - p.x0, ph = p.y1 - p.y0;
  const float a1 = pw * ph, a2 = (t.x1 - t.x0) * (t.y1 - t.y0);
  const float iwr = fminf(p.x1, t.x1) - fmaxf(p.x0, t.x0), ihr = fminf(p.y1, t.y1) - fmaxf(p.y0, t.y0);
  const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
  const float inter = iw * ih, uni = a1 + a2 - inter;
  const float ewr = fmaxf(p.x1, t.x1) - fminf(p.x0, t.x0), ehr = fmaxf(p.y1, t.y1) - fminf(p.y0, t.y0);
  const float ew = fmaxf(ewr, 0.f), eh = fmaxf(ehr, 0.f);
  const float ac = ew * eh;
  // derivatives with respect to the corners (x0, y0, x1, y1) of the first box
  const float diw[4] = {(iwr > 0.f && p.x0 > t.x0) ? -1.f : 0.f, 0.f, (iwr > 0.f && p.x1 < t.x1) ? 1.f : 0.f, 0.f};
  const float dih[4] = {0.f, (ihr > 0.f && p.y0 > t.y0) ? -1.f : 0.f, 0.f, (ihr > 0.f && p.y1 < t.y1) ? 1.f : 0.f};
  const float dew[4] = {(ewr > 0.f && p.x0 < t.x0) ? -1.f : 0.f, 0.f, (ewr > 0.f && p.x1 > t.x1) ? 1.f : 0.f, 0.f};
  const float deh[4] = {0.f, (ehr > 0.f && p.y0 < t.y0) ? -1.f : 0.f, 0.f, (ehr > 0.f && p.y1 > t.y1) ? 1.f : 0.f};
  const float da1[4] = {-ph, -pw, ph, pw};
  float gc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dinter = diw[k] * ih + iw * dih[k];
    const float duni = da1[k] - dinter;
    const float dac = dew[k] * eh + ew * deh[k];
    // giou = inter / uni - 1 + uni / ac
    gc[k] = (dinter * uni - inter * duni) / (uni * uni) + (duni * ac - uni * dac) / (ac * ac);
  }
  g[0] = gc[0] + gc[2];
  g[1] = gc[1] + gc[3];
  g[2] = 0.5f * (gc[2] - gc[0]);
  g[3] = 0.5f * (gc[3] - gc[1]);
}

// row m of the gathered [B*Q, D] view = row T - Q + q of image b
__device__ __forceinline__ long det_src_row(long m, int T, int Q) {
  const long b = m / Q;
  return b * T + (T - Q) + (m - b * Q);
}

// ---------------------------------------------------------------------------------------------------------------- decoder
__global__ __launch_bounds__(256) void det_heads_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wc,
                                                            const float* __restrict__ bc, const float* __restrict__ wb,
                                                            const float* __restrict__ bb, float* __restrict__ logits,
                                                            float* __restrict__ boxes, long M, int T, int Q, int D, int C1) {
  extern __shared__ float xs[];                            // [DET_ROWS][D]
  const long m0 = (long)blockIdx.x * DET_ROWS;
  for (int i = threadIdx.x; i < DET_ROWS * D; i += 256) {
    const int r = i / D, d = i - r * D;
    const long m = m0 + r;
    xs[i] = m < M ? x[det_src_row(m, T, Q) * D + d] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = C1 + 4;
  for (int n = wave; n < N; n += 4) {
    const float* w = n < C1 ? wc + (long)n * D : wb + (long)(n - C1) * D;
    float acc[DET_ROWS];
#pragma unroll
    for (int r = 0; r < DET_ROWS; ++r) acc[r] = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float wv = w[d];
#pragma unroll
      for (int r = 0; r < DET_ROWS; ++r) acc[r] = fmaf(xs[r * D + d], wv, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < DET_ROWS; ++r) acc[r] = wave_sum(acc[r]);
    if (lane == 0) {
      const float bias = n < C1 ? bc[n] : bb[n - C1];
#pragma unroll
      for (int r = 0; r < DET_ROWS; ++r) {
        const long m = m0 + r;
        if (m < M) {
          const float v = acc[r] + bias;
          if (n < C1) logits[m * C1 + n] = v;
          else boxes[m * 4 + (n - C1)] = 1.f / (1.f + expf(-v));       // bbox_embed(x).sigmoid()
        }
      }
    }
  }
}

// d(pre-activation) of output column n of row m: the class head's gradient as it is, the box head's times sigmoid' = s (1 - s)
__device__ __forceinline__ float det_dy(const float* __restrict__ dlogits, const float* __restrict__ dboxes,
                                        const float* __restrict__ boxes, long m, int n, int C1) {
  if (n < C1) return dlogits ? dlogits[m * C1 + n] : 0.f;
  if (!dboxes) return 0.f;
  const float s = boxes[m * 4 + (n - C1)];
  return dboxes[m * 4 + (n - C1)] * s * (1.f - s);
}

__global__ __launch_bounds__(256) void det_heads_dx_kernel(const float* __restrict__ wc, const float* __restrict__ wb,
                                                           const float* __restrict__ boxes, const float* __restrict__ dlogits,
                                                           const float* __restrict__ dboxes, float* __restrict__ dx, long M,
                                                           int T, int Q, int D, int C1) {
  __shared__ float dys[DET_ROWS][DET_NMAX];
  const long m0 = (long)blockIdx.x * DET_ROWS;
  const int N = C1 + 4;
  for (int i = threadIdx.x; i < DET_ROWS * N; i += 256) {
    const int r = i / N, n = i - r * N;
    const long m = m0 + r;
    dys[r][n] = m < M ? det_dy(dlogits, dboxes, boxes, m, n, C1) : 0.f;
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 256) {
    float acc[DET_ROWS];
#pragma unroll
    for (int r = 0; r < DET_ROWS; ++r) acc[r] = 0.f;
    for (int n = 0; n < N; ++n) {
      const float wv = n < C1 ? wc[(long)n * D + d] : wb[(long)(n - C1) * D + d];
#pragma unroll
      for (int r = 0; r < DET_ROWS; ++r) acc[r] = fmaf(dys[r][n], wv, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < DET_ROWS; ++r) {
      const long m = m0 + r;
      if (m < M) dx[det_src_row(m, T, Q) * D + d] = acc[r];
    }
  }
}

// partial[s][n][0..D) = sum over the rows of slab s of dY[m, n] X[m, :], partial[s][n][D] = the same sum of dY[m, n] (bias)
__global__ __launch_bounds__(256) void det_heads_dw_kernel(const float* __restrict__ x, const float* __restrict__ boxes,
                                                           const float* __restrict__ dlogits, const float* __restrict__ dboxes,
                                                           float* __restrict__ partial, long M, int rows_per_slab, int T, int Q,
                                                           int D, int C1) {
  const int N = C1 + 4;
  const int n0 = blockIdx.y * DET_DW_NT, s = blockIdx.z;
  const int d = blockIdx.x * 256 + threadIdx.x;
  const long mlo = (long)s * rows_per_slab;
  long mhi = mlo + rows_per_slab;
  if (mhi > M) mhi = M;
  float acc[DET_DW_NT], bsum[DET_DW_NT];
#pragma unroll
  for (int j = 0; j < DET_DW_NT; ++j) acc[j] = bsum[j] = 0.f;
  for (long m = mlo; m < mhi; ++m) {
    const float xv = d < D ? x[det_src_row(m, T, Q) * D + d] : 0.f;
#pragma unroll
    for (int j = 0; j < DET_DW_NT; ++j) {
      const float dy = n0 + j < N ? det_dy(dlogits, dboxes, boxes, m, n0 + j, C1) : 0.f;      // uniform over the workgroup
      acc[j] = fmaf(dy, xv, acc[j]);
      bsum[j] += dy;
    }
  }
#pragma unroll
  for (int j = 0; j < DET_DW_NT; ++j) {
    if (n0 + j >= N) continue;
    float* row = partial + ((long)s * N + (n0 + j)) * (D + 1);
    if (d < D) row[d] = acc[j];
    if (d == 0) row[D] = bsum[j];
  }
}

__global__ __launch_bounds__(256) void det_heads_dw_sum_kernel(const float* __restrict__ partial, int S, float* __restrict__ dwc,
                                                               float* __restrict__ dbc, float* __restrict__ dwb,
                                                               float* __restrict__ dbb, int D, int C1) {
  const int N = C1 + 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * (D + 1)) return;
  const int n = (int)(i / (D + 1)), d = (int)(i - (long)n * (D + 1));
  float t = 0.f;
  for (int s = 0; s < S; ++s) t += partial[((long)s * N + n) * (D + 1) + d];          // slab order: deterministic
  if (d < D) {
    if (n < C1) dwc[(long)n * D + d] = t;
    else dwb[(long)(n - C1) * D + d] = t;
  } else {
    if (n < C1) dbc[n] = t;
    else dbb[n - C1] = t;
  }
}

// --------------------------------------------------------------------------------------------------------- sequence assembly
__global__ __launch_bounds__(256) void det_append_fwd_kernel(const float* __restrict__ x, const float* __restrict__ det,
                                                             const float* __restrict__ pos, float* __restrict__ out, long total,
                                                             int T0, int Q, int D) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int T = T0 + Q;
  const long row = i / D;
  const int d = (int)(i - row * D);
  const long b = row / T;
  const int t = (int)(row - b * T);
  out[i] = t < T0 ? x[(b * T0 + t) * D + d] : det[(long)(t - T0) * D + d] + pos[(long)(t - T0) * D + d];
}

// elements [0, B*T0*D): the copy dx = dout[:, :T0]; elements beyond: (q, d) sums over the batch in batch order
__global__ __launch_bounds__(256) void det_append_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dx,
                                                             float* __restrict__ ddet, float* __restrict__ dpos, int B, int T0,
                                                             int Q, int D) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long ncopy = (long)B * T0 * D, T = T0 + Q;
  if (i < ncopy) {
    const long row = i / D;
    const int d = (int)(i - row * D);
    const long b = row / T0;
    const int t = (int)(row - b * T0);
    dx[i] = dout[(b * T + t) * D + d];
  } else if (i < ncopy + (long)Q * D) {
    const long j = i - ncopy;
    const int q = (int)(j / D), d = (int)(j - (long)q * D);
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dout[((long)b * T + T0 + q) * D + d];
    ddet[j] = s;
    dpos[j] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------------ matcher
// out + Q * toff[b]: the [Q, T_b] block of image b, row-major
__global__ __launch_bounds__(64) void det_cost_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                      const int64_t* __restrict__ labels, const float* __restrict__ tboxes,
                                                      const int32_t* __restrict__ toff, float* __restrict__ out, float cost_class,
                                                      float cost_bbox, float cost_giou, int Q, int C1) {
  const int b = blockIdx.y, q = blockIdx.x, lane = threadIdx.x;
  const int t0 = toff[b], nt = toff[b + 1] - t0;
  if (nt <= 0) return;
  const float* l = logits + ((long)b * Q + q) * C1;
  float mx = -INFINITY;
  for (int c = lane; c < C1; c += 64) mx = fmaxf(mx, l[c]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int c = lane; c < C1; c += 64) s += expf(l[c] - mx);
  s = wave_sum(s);
  const float inv = 1.f / s;
  const float* pb = boxes + ((long)b * Q + q) * 4;
  const float p0 = pb[0], p1 = pb[1], p2 = pb[2], p3 = pb[3];
  const float pbox[4] = {p0, p1, p2, p3};
  const DetBox px = det_xyxy(pbox);
  float* o = out + (long)Q * t0 + (long)q * nt;
  for (int t = lane; t < nt; t += 64) {
    const int64_t lab = labels[t0 + t];
    const float prob = (lab >= 0 && lab < C1) ? expf(l[lab] - mx) * inv : __builtin_nanf("");   // never an out-of-range index
    const float* tb = tboxes + (long)(t0 + t) * 4;
    const float tbox[4] = {tb[0], tb[1], tb[2], tb[3]};
    const float l1 = (fabsf(p0 - tbox[0]) + fabsf(p1 - tbox[1])) + (fabsf(p2 - tbox[2]) + fabsf(p3 - tbox[3]));
    const float g = det_giou(px, det_xyxy(tbox));
    o[t] = cost_bbox * l1 - cost_class * prob - cost_giou * g;
  }
}

// per-query target class / box from the matching: match[i] = flat index of query i's target, or -1 (then: no_object, zeros)
__global__ __launch_bounds__(256) void det_assign_kernel(const int32_t* __restrict__ match, const int64_t* __restrict__ labels,
                                                         const float* __restrict__ tboxes, int64_t* __restrict__ tgt_class,
                                                         float* __restrict__ tgt_box, long n, long ntargets, int no_object) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = match[i];
  const bool hit = j >= 0 && j < ntargets;
  tgt_class[i] = hit ? labels[j] : (int64_t)no_object;
#pragma unroll
  for (int k = 0; k < 4; ++k) tgt_box[i * 4 + k] = hit ? tboxes[(long)j * 4 + k] : 0.f;
}

// Rectangular minimum-cost assignment of one image's [Q, T_b] block: the shortest-augmenting-path method of
// scipy.optimize.linear_sum_assignment (Crouse 2016), fp64 duals and path costs over the fp32 costs, in the same operation order.
// One wave per image.  The smaller side is the rows (scipy transposes when T_b < Q); lane l owns columns l, l + 64, ...: it alone
// reads and writes their path cost, predecessor and visited flag inside a search, so a Dijkstra step is a lane-parallel
// relaxation of the unvisited columns, a wave arg-min and nothing else -- the two barriers per row sit around the dual update and
// the augmentation, which cross lanes.  Arg-min order: smaller value, then an unassigned column, then the lower index
// (deterministic; scipy's order differs, so the assignment equals scipy's wherever the optimum is unique).
// Every loop bound comes from the sizes: nr rows, at most nc steps per search (a step visits one more column), at most nr hops
// per augmentation; NaN and -inf are screened while the block is staged, before the solve.
// LDS: u[nr_max] v[nc_max] sp[nc_max] (fp64) | path[nc_max] row4col[nc_max] col4row[nr_max] (int32) | visited[nc_max] (bytes) |
// the cost block (cost_cap floats), rows unit-stride, when it fits; otherwise the block is read from global memory.
// Known costs outside the solve, left as they are because the serial search dominates: the transposed staging (T_b < Q) divides
// once per element and writes LDS at a stride of Q words (a 4-way bank conflict at Q = 100), and the global-memory fallback of a
// transposed block reads at a stride of T_b floats (uncoalesced).  A tiled transpose would remove both.
constexpr int DET_MATCH_MAX = 1024;
constexpr int DET_MATCH_ASSIGNED = 1 << 20;      // arg-min key: assigned flag | column << 10 | the column's row

__host__ __device__ inline size_t det_match_state_bytes(int nr_max, int nc_max) {
  return ((size_t)nr_max * 12 + (size_t)nc_max * 25 + 15) & ~(size_t)15;
}

__global__ __launch_bounds__(64) void det_match_kernel(const float* __restrict__ cost, const int32_t* __restrict__ toff,
                                                       int32_t* __restrict__ match, int32_t* __restrict__ status, int Q, int max_t,
                                                       int nr_max, int nc_max, int cost_cap) {
  extern __shared__ double det_match_lds[];
  double* u = det_match_lds;                                // [nr_max] row duals
  double* v = u + nr_max;                                   // [nc_max] column duals
  double* sp = v + nc_max;                                  // [nc_max] shortest path cost to a column in this search
  int* path = (int*)(sp + nc_max);                          // [nc_max] the row a column was reached from
  int* row4col = path + nc_max;                             // [nc_max] the column's row, or -1
  int* col4row = row4col + nc_max;                          // [nr_max] the row's column, or -1
  unsigned char* seen = (unsigned char*)(col4row + nr_max); // [nc_max] visited in this search
  float* cst = (float*)((char*)det_match_lds + det_match_state_bytes(nr_max, nc_max));

  const int b = blockIdx.x, lane = threadIdx.x;
  const int t0 = toff[b], nt = toff[b + 1] - t0;
  int32_t* m = match + (long)b * Q;
  if (nt <= 0 || nt > max_t) {                              // no targets: solved; a count outside [0, max_t]: invalid input
    for (int q = lane; q < Q; q += 64) m[q] = -1;
    if (lane == 0) status[b] = nt == 0 ? 0 : 1;
    return;
  }
  const float* g = cost + (long)Q * t0;
  const bool tr = nt < Q;                                   // rows = targets, columns = queries
  const int nr = tr ? nt : Q, nc = tr ? Q : nt;
  const int n = Q * nt;
  const bool in_lds = n <= cost_cap;

  bool bad = false;
  for (int idx = lane; idx < n; idx += 64) {
    const float c = g[idx];
    bad |= !(c > -INFINITY);                                // NaN or -inf
    if (in_lds) {
      if (tr) {
        const int q = idx / nt, t = idx - q * nt;
        cst[t * Q + q] = c;
      } else {
        cst[idx] = c;
      }
    }
  }
  if (__any(bad)) {
    for (int q = lane; q < Q; q += 64) m[q] = -1;
    if (lane == 0) status[b] = 1;
    return;
  }
  for (int i = lane; i < nr; i += 64) { u[i] = 0.0; col4row[i] = -1; }
  for (int j = lane; j < nc; j += 64) { v[j] = 0.0; row4col[j] = -1; }
  __syncthreads();

  const double inf = (double)INFINITY;
  int st = 0;
  for (int cur = 0; cur < nr; ++cur) {
    for (int j = lane; j < nc; j += 64) { sp[j] = inf; seen[j] = 0; }
    double minv = 0.0;
    int i = cur, sink = -1;
    for (int step = 0; step < nc; ++step) {
      const double ui = u[i];
      double bv = inf;
      int bk = 0x7fffffff;
      for (int j = lane; j < nc; j += 64) {
        if (seen[j]) continue;
        const float c = in_lds ? cst[i * nc + j] : (tr ? g[(long)j * nt + i] : g[(long)i * nt + j]);
        const double r = ((minv + (double)c) - ui) - v[j];
        double s = sp[j];
        if (r < s) { s = r; sp[j] = r; path[j] = i; }
        const int rw = row4col[j];
        const int k = (rw >= 0 ? (DET_MATCH_ASSIGNED | rw) : 0) | (j << 10);
        if (s < bv || (s == bv && k < bk)) { bv = s; bk = k; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int ok = __shfl_xor(bk, o, 64);
        if (ov < bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
      }
      if (!(bv < inf)) break;                               // only forbidden pairs are left: infeasible
      minv = bv;
      const int j = (bk >> 10) & (DET_MATCH_MAX - 1);
      if ((j & 63) == lane) seen[j] = 1;
      if (bk & DET_MATCH_ASSIGNED) {
        i = bk & (DET_MATCH_MAX - 1);
      } else {
        sink = j;
        break;
      }
    }
    if (sink < 0) { st = 2; break; }
    // dual update: u[cur] += minv; for the other visited rows i (= row4col of a visited column j) u[i] += minv - sp[j];
    // for the visited columns v[j] -= minv - sp[j]
    if (lane == 0) u[cur] += minv;
    for (int j = lane; j < nc; j += 64) {
      if (!seen[j]) continue;
      const double d = minv - sp[j];
      v[j] -= d;
      const int r = row4col[j];
      if (r >= 0) u[r] += d;
    }
    __syncthreads();
    if (lane == 0) {                                        // augment along the predecessors back to cur
      int j = sink;
      for (int hop = 0; hop < nr; ++hop) {
        const int r = path[j];
        row4col[j] = r;
        const int jn = col4row[r];
        col4row[r] = j;
        j = jn;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
  for (int q = lane; q < Q; q += 64) {
    int t = -1;
    if (st == 0) t = tr ? row4col[q] : col4row[q];
    m[q] = t >= 0 ? t0 + t : -1;
  }
  if (lane == 0) status[b] = st;
}

// ---------------------------------------------------------------------------------------------------------------- criterion
constexpr int DET_NSTAT = 7;

__global__ __launch_bounds__(256) void det_loss_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                           const int64_t* __restrict__ tgt_class, const float* __restrict__ tgt_box,
                                                           const float* __restrict__ weight, const int32_t* __restrict__ tcount,
                                                           float* __restrict__ lse, float* __restrict__ stats, float inv_num_boxes,
                                                           int B, int Q, int C1) {
  extern __shared__ int card[];                             // [B]: queries whose arg-max is not the last class
  __shared__ float red[DET_NSTAT][4];
  for (int b = threadIdx.x; b < B; b += 256) card[b] = 0;
  __syncthreads();
  // ce numerator, ce denominator, L1 sum, (1 - GIoU) sum, matched queries, matched queries whose arg-max is their class, bad classes
  float v[DET_NSTAT];
#pragma unroll
  for (int k = 0; k < DET_NSTAT; ++k) v[k] = 0.f;
  const long n = (long)B * Q;
  for (long i = threadIdx.x; i < n; i += 256) {
    const float* l = logits + i * C1;
    float mx = -INFINITY;
    int am = 0;
    for (int c = 0; c < C1; ++c) {
      const float x = l[c];
      if (x > mx) { mx = x; am = c; }
    }
    float s = 0.f;
    for (int c = 0; c < C1; ++c) s += expf(l[c] - mx);
    const float ls = mx + logf(s);
    lse[i] = ls;
    if (am != C1 - 1) atomicAdd(&card[i / Q], 1);
    const int64_t t = tgt_class[i];
    if (t < 0 || t >= C1) { v[6] += 1.f; continue; }
    const float w = weight[t];
    v[0] += w * (ls - l[t]);
    v[1] += w;
    if (t != C1 - 1) {                                      // a matched query
      v[4] += 1.f;
      v[5] += am == (int)t ? 1.f : 0.f;
      const float* pb = boxes + i * 4;
      const float* tb = tgt_box + i * 4;
      const float p[4] = {pb[0], pb[1], pb[2], pb[3]}, g[4] = {tb[0], tb[1], tb[2], tb[3]};
      v[2] += (fabsf(p[0] - g[0]) + fabsf(p[1] - g[1])) + (fabsf(p[2] - g[2]) + fabsf(p[3] - g[3]));
      v[3] += 1.f - det_giou(det_xyxy(p), det_xyxy(g));
    }
  }
#pragma unroll
  for (int k = 0; k < DET_NSTAT; ++k) {
    v[k] = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();                                          // also: every card[] atomic has landed
  float ce = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) ce += fabsf((float)card[b] - (float)tcount[b]);
  ce = wave_sum(ce);
  __shared__ float red_card[4];
  if ((threadIdx.x & 63) == 0) red_card[threadIdx.x >> 6] = ce;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[DET_NSTAT];
#pragma unroll
    for (int k = 0; k < DET_NSTAT; ++k) t[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
    stats[0] = t[6] > 0.f ? __builtin_nanf("") : t[0] / t[1];                 // weighted mean (torch's semantics)
    stats[1] = t[2] * inv_num_boxes;
    stats[2] = t[3] * inv_num_boxes;
    stats[3] = t[4] > 0.f ? 100.f - 100.f * t[5] / t[4] : 100.f;              // 100 - accuracy(...) (0 when nothing is matched)
    stats[4] = ((red_card[0] + red_card[1]) + (red_card[2] + red_card[3])) / (float)B;
    stats[5] = t[1];
    stats[6] = t[4];
    stats[7] = t[6];
  }
}

__global__ __launch_bounds__(256) void det_loss_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                           const int64_t* __restrict__ tgt_class, const float* __restrict__ tgt_box,
                                                           const float* __restrict__ weight, const float* __restrict__ lse,
                                                           const float* __restrict__ stats, const float* __restrict__ g_ce,
                                                           const float* __restrict__ g_bbox, const float* __restrict__ g_giou,
                                                           float* __restrict__ dlogits, float* __restrict__ dboxes,
                                                           float inv_num_boxes, long n, int C1) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float gce = g_ce ? *g_ce : 0.f, gl1 = (g_bbox ? *g_bbox : 0.f) * inv_num_boxes,
              ggi = (g_giou ? *g_giou : 0.f) * inv_num_boxes;
  const int64_t t = tgt_class[i];
  const bool ok = t >= 0 && t < C1;
  const float* l = logits + i * C1;
  const float ls = lse[i];
  const float k = ok ? gce * weight[t] / stats[5] : 0.f;
  for (int c = 0; c < C1; ++c) dlogits[i * C1 + c] = k * (expf(l[c] - ls) - (c == (int)t ? 1.f : 0.f));
  float db[4] = {0.f, 0.f, 0.f, 0.f};
  if (ok && t != C1 - 1) {
    const float* pb = boxes + i * 4;
    const float* tb = tgt_box + i * 4;
    const float p[4] = {pb[0], pb[1], pb[2], pb[3]}, g[4] = {tb[0], tb[1], tb[2], tb[3]};
    float gg[4];
    det_giou_grad(det_xyxy(p), det_xyxy(g), gg);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = p[j] - g[j];
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      db[j] = gl1 * sgn - ggi * gg[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) dboxes[i * 4 + j] = db[j];
}

// ------------------------------------------------------------------------------------------------------------- post-process
__global__ __launch_bounds__(256) void det_postprocess_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                              const float* __restrict__ sizes, float* __restrict__ scores,
                                                              int64_t* __restrict__ labels, float* __restrict__ out, long n,
                                                              int Q, int C1) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* l = logits + i * C1;
  float mx = -INFINITY, best = -INFINITY;
  int am = 0;
  for (int c = 0; c < C1; ++c) {
    const float x = l[c];
    mx = fmaxf(mx, x);
    if (c < C1 - 1 && x > best) { best = x; am = c; }
  }
  float s = 0.f;
  for (int c = 0; c < C1; ++c) s += expf(l[c] - mx);
  scores[i] = expf(best - mx) / s;
  labels[i] = am;
  const float* pb = boxes + i * 4;
  const float p[4] = {pb[0], pb[1], pb[2], pb[3]};
  const DetBox bx = det_xyxy(p);
  const float ih = sizes[(i / Q) * 2], iw = sizes[(i / Q) * 2 + 1];
  out[i * 4 + 0] = bx.x0 * iw;
  out[i * 4 + 1] = bx.y0 * ih;
  out[i * 4 + 2] = bx.x1 * iw;
  out[i * 4 + 3] = bx.y1 * ih;
}

inline int det_slabs(long M) {
  long s = (M + DET_DW_SLAB - 1) / DET_DW_SLAB;
  return (int)(s < 1 ? 1 : (s > DET_DW_MAXSLABS ? DET_DW_MAXSLABS : s));
}

inline bool det_dims_ok(int B, int Q, int C1) { return B > 0 && Q > 0 && C1 >= 2 && B <= 65535 && (long)B * Q < (1l << 30); }

}  // namespace

extern "C" int mv_det_heads_fwd(const float* x, const float* w_cls, const float* b_cls, const float* w_box, const float* b_box,
                                float* logits, float* boxes, int B, int T, int Q, int D, int C1, mv_stream_t stream) {
  MV_REQUIRE(det_dims_ok(B, Q, C1) && T >= Q && D > 0 && C1 + 4 <= DET_NMAX, MV_ERR_SHAPE);
  const size_t lds = (size_t)DET_ROWS * D * sizeof(float);
  MV_REQUIRE(lds <= DET_LDS_LIMIT, MV_ERR_UNSUPPORTED);
  const long M = (long)B * Q;
  return mv_launch<det_heads_fwd_kernel>(MV_HERE, mv_cdiv(M, DET_ROWS), 256, lds, (hipStream_t)stream, x, w_cls, b_cls, w_box,
                                         b_box, logits, boxes, M, T, Q, D, C1);
}

extern "C" size_t mv_det_heads_bwd_workspace_bytes(int B, int Q, int D, int C1) {
  if (B <= 0 || Q <= 0 || D <= 0 || C1 <= 0) return 0;
  return (size_t)det_slabs((long)B * Q) * (size_t)(C1 + 4) * (size_t)(D + 1) * sizeof(float);
}

extern "C" int mv_det_heads_bwd(const float* x, const float* w_cls, const float* w_box, const float* boxes, const float* dlogits,
                                const float* dboxes, float* dx, float* dw_cls, float* db_cls, float* dw_box, float* db_box,
                                void* workspace, size_t workspace_bytes, int B, int T, int Q, int D, int C1, mv_stream_t stream) {
  MV_REQUIRE(det_dims_ok(B, Q, C1) && T >= Q && D > 0 && C1 + 4 <= DET_NMAX, MV_ERR_SHAPE);
  MV_REQUIRE(workspace_bytes >= mv_det_heads_bwd_workspace_bytes(B, Q, D, C1) && mv_aligned16(workspace), MV_ERR_ALIGN);
  const long M = (long)B * Q;
  const int N = C1 + 4;
  hipStream_t s = (hipStream_t)stream;
  if (dx)
    if (int rc = mv_launch<det_heads_dx_kernel>(MV_HERE, mv_cdiv(M, DET_ROWS), 256, 0, s, w_cls, w_box, boxes, dlogits, dboxes, dx, M, T, Q, D, C1))
      return rc;
  const int S = det_slabs(M);
  const int rows_per_slab = (int)((M + S - 1) / S);
  float* partial = (float*)workspace;
  if (int rc = mv_launch<det_heads_dw_kernel>(MV_HERE, dim3(mv_cdiv(D, 256), mv_cdiv(N, DET_DW_NT), S), 256, 0, s, x, boxes, dlogits, dboxes,
                                              partial, M, rows_per_slab, T, Q, D, C1))
    return rc;
  return mv_launch<det_heads_dw_sum_kernel>(MV_HERE, mv_cdiv((long)N * (D + 1), 256), 256, 0, s, partial, S, dw_cls, db_cls, dw_box, db_box,
                                            D, C1);
}

extern "C" int mv_det_append_fwd(const float* x, const float* det, const float* pos, float* out, int B, int T0, int Q, int D,
                                 mv_stream_t stream) {
  MV_REQUIRE(B > 0 && T0 > 0 && Q > 0 && D > 0, MV_ERR_SHAPE);
  const long total = (long)B * (T0 + Q) * D;
  MV_REQUIRE(total / 256 < 0x7fffffffl, MV_ERR_SHAPE);
  return mv_launch<det_append_fwd_kernel>(MV_HERE, mv_cdiv(total, 256), 256, 0, (hipStream_t)stream, x, det, pos, out, total, T0, Q,
                                          D);
}

extern "C" int mv_det_append_bwd(const float* dout, float* dx, float* ddet, float* dpos, int B, int T0, int Q, int D,
                                 mv_stream_t stream) {
  MV_REQUIRE(B > 0 && T0 > 0 && Q > 0 && D > 0, MV_ERR_SHAPE);
  const long total = (long)B * T0 * D + (long)Q * D;
  MV_REQUIRE(total / 256 < 0x7fffffffl, MV_ERR_SHAPE);
  return mv_launch<det_append_bwd_kernel>(MV_HERE, mv_cdiv(total, 256), 256, 0, (hipStream_t)stream, dout, dx, ddet, dpos, B, T0, Q,
                                          D);
}

extern "C" int mv_det_cost(const float* logits, const float* boxes, const int64_t* labels, const float* tboxes,
                           const int32_t* toff, float* out, float cost_class, float cost_bbox, float cost_giou, int B, int Q,
                           int C1, mv_stream_t stream) {
  MV_REQUIRE(det_dims_ok(B, Q, C1), MV_ERR_SHAPE);
  return mv_launch<det_cost_kernel>(MV_HERE, dim3(Q, B), 64, 0, (hipStream_t)stream, logits, boxes, labels, tboxes, toff, out,
                                    cost_class, cost_bbox, cost_giou, Q, C1);
}

extern "C" int mv_det_match(const float* cost, const int32_t* toff, int32_t* match, int32_t* status, int B, int Q, int max_t,
                            mv_stream_t stream) {
  MV_REQUIRE(det_dims_ok(B, Q, 2) && max_t >= 0, MV_ERR_SHAPE);
  MV_REQUIRE(Q <= DET_MATCH_MAX && max_t <= DET_MATCH_MAX, MV_ERR_UNSUPPORTED);
  const int nr_max = Q < max_t ? Q : max_t, nc_max = Q < max_t ? max_t : Q;
  const size_t state = det_match_state_bytes(nr_max, nc_max);
  size_t cap = (DET_LDS_LIMIT - state) / sizeof(float);
  if ((size_t)Q * max_t < cap) cap = (size_t)Q * max_t;
  return mv_launch<det_match_kernel>(MV_HERE, B, 64, state + cap * sizeof(float), (hipStream_t)stream, cost, toff, match, status, Q,
                                     max_t, nr_max, nc_max, (int)cap);
}

extern "C" int mv_det_assign(const int32_t* match, const int64_t* labels, const float* tboxes, int64_t* tgt_class, float* tgt_box,
                             long n, long ntargets, int no_object, mv_stream_t stream) {
  MV_REQUIRE(n > 0 && n < (1l << 30) && ntargets >= 0 && no_object >= 0, MV_ERR_SHAPE);
  return mv_launch<det_assign_kernel>(MV_HERE, mv_cdiv(n, 256), 256, 0, (hipStream_t)stream, match, labels, tboxes, tgt_class,
                                      tgt_box, n, ntargets, no_object);
}

extern "C" int mv_det_loss_fwd(const float* logits, const float* boxes, const int64_t* tgt_class, const float* tgt_box,
                               const float* weight, const int32_t* tcount, float* lse, float* stats, float inv_num_boxes, int B,
                               int Q, int C1, mv_stream_t stream) {
  MV_REQUIRE(det_dims_ok(B, Q, C1), MV_ERR_SHAPE);
  MV_REQUIRE((size_t)B * sizeof(int) <= DET_LDS_LIMIT / 2, MV_ERR_UNSUPPORTED);
  return mv_launch<det_loss_fwd_kernel>(MV_HERE, 1, 256, (size_t)B * sizeof(int), (hipStream_t)stream, logits, boxes, tgt_class,
                                        tgt_box, weight, tcount, lse, stats, inv_num_boxes, B, Q, C1);
}

extern "C" int mv_det_loss_bwd(const float* logits, const float* boxes, const int64_t* tgt_class, const float* tgt_box,
                               const float* weight, const float* lse, const float* stats, const float* g_ce, const float* g_bbox,
                               const float* g_giou, float* dlogits, float* dboxes, float inv_num_boxes, int B, int Q, int C1,
                               mv_stream_t stream) {
  MV_REQUIRE(det_dims_ok(B, Q, C1), MV_ERR_SHAPE);
  const long n = (long)B * Q;
  return mv_launch<det_loss_bwd_kernel>(MV_HERE, mv_cdiv(n, 256), 256, 0, (hipStream_t)stream, logits, boxes, tgt_class, tgt_box,
                                        weight, lse, stats, g_ce, g_bbox, g_giou, dlogits, dboxes, inv_num_boxes, n, C1);
}

extern "C" int mv_det_postprocess(const float* logits, const float* boxes, const float* sizes, float* scores, int64_t* labels,
                                  float* out_boxes, int B, int Q, int C1, mv_stream_t stream) {
  MV_REQUIRE(det_dims_ok(B, Q, C1), MV_ERR_SHAPE);
  const long n = (long)B * Q;
  return mv_launch<det_postprocess_kernel>(MV_HERE, mv_cdiv(n, 256), 256, 0, (hipStream_t)stream, logits, boxes, sizes, scores,
                                           labels, out_boxes, n, Q, C1);
}
