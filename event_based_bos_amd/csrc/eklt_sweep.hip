// eklt_sweep.hip -- the reference's sampled EKLT solvers, patch_eklt (src/solver/patch_eklt.py) and generative_max_likelihood
// (src/solver/generative_max_likelihood.py), as one sweep in float64: every box (a patch, or the one ROI) is scored against the
// event histogram under every hypothesis (v_x, v_y, p_x, p_y) of a table, and the best hypothesis of a box wins.
//
//   Gx = T_p(gx), Gy = T_p(gy);  P0 = v_x Gx + v_y Gy on the box (|P0| if no_polarity, * we[box]);  P = P0 / (|P0|_F + 1e-4)
//   Q = q[box] / |q[box]|_F;     cost = w_dn max_c sum_r |P - Q|
//
// T_p is cv2.warpPerspective of the WHOLE image by the translation (p_x rows, p_y columns), INTER_LINEAR, BORDER_CONSTANT 0, in
// OpenCV's classic path: the source coordinate is rounded to 1/32 pixel, so that a hypothesis's warp is one integer shift
// (s_r, s_c) plus the four float32 table weights of its two fractions for every pixel of the image:
//   G(r, c) = ((g(r + s_r, c + s_c) w00 + g(r + s_r, c + s_c + 1) w01) + g(r + s_r + 1, c + s_c) w10) + g(r + s_r + 1, c + s_c + 1) w11
// with g = 0 outside the image (and the image's own values outside the box: the warp precedes the crop).  The host derives
// (s_r, s_c, w..) per hypothesis once per call (eklt_hypothesis).  Every product and sum is rounded on its own (no contraction).
//
// Launches of one call, all on the caller's stream, no atomics, every reduction in a fixed order:
//   eklt_qnorm          one workgroup per (box, window): |q[box]|_F -> qn (0 = the box is not evaluated: unselected, not inside
//                       the image or larger than the call's ph x pw, or its norm is 0 or NaN)
//   eklt_sweep_patch    the PATCH route.  One workgroup per (box, chunk of 256 hypotheses, window): the box of gx, gy with a halo
//                       of max |shift| + 1 pixels, we[box] and Q go into LDS once; then ONE hypothesis per thread: pass 1 the
//                       sum of P0^2 over the box in row-major order, pass 2 the column sums of |P - Q| and their maximum.  A
//                       hypothesis's cost is a function of the box and the hypothesis alone (one thread, serial order).
//   eklt_sweep_roi      the ROI route, for boxes whose planes do not fit in LDS (up to the full image).  One workgroup per
//                       (hypothesis, box, window) reading global memory: pass 1 strided partial sums and a fixed tree, pass 2 one
//                       column per thread and a fixed tree of maxima.
//   eklt_argmin         one thread per (box, window): the partial winners in chunk order; strict <, so the lowest index wins a
//                       tie; a NaN cost never wins (index -1 and cost +inf where nothing won)
//
// LDS of the patch route: 8 B x (2 (ph + 2 halo)(pw + 2 halo) + 2 ph pw) <= 160 KiB - 4 KiB (ebos_eklt_sweep_fits).
//
// ebos_eklt_patch_flow_batch_f64: the winners' (v_x, v_y) into the patch grid (0 where nothing won), then the upsample of
// interpolate_dense_flow_from_patch_numpy (edge pad, bilinear x slide, centre crop) with the dependent solver's device code
// (gml_upsample.h).
#pragma clang fp contract(off)

#include <math.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "gml_upsample.h"

namespace ebos {
namespace {

constexpr int kSweepBlock = 256;
constexpr size_t kSweepLdsBytes = 160 * 1024 - 4096;   // the planes; the rest is the reduction's
constexpr int kSweepMaxShift = 1 << 20;                // beyond any image: every tap is outside
constexpr int kSweepMaxWindows = 65535;                // gridDim.z

struct Hyp {
  double vx, vy;
  double w00, w01, w10, w11;   // the float32 table weights (1 - fy, fy) x (1 - fx, fx), widened
  int sr, sc;                  // integer shift of rows / columns
};

// (v_x, v_y, p_x, p_y) -> the warp's constants, exactly as the classic path rounds: the inverse of [[1, 0, p_y], [0, 1, p_x],
// [0, 0, 1]] has -p_y, -p_x in its last column, and destination (x, y) reads source 32 (x - p_y) rounded half to even.
Hyp eklt_hypothesis(const double* h) {
  Hyp o;
  o.vx = h[0];
  o.vy = h[1];
  const double px = h[2], py = h[3];
  if (!std::isfinite(px) || !std::isfinite(py)) {   // no warp exists: the cost is NaN
    o.vx = o.vy = NAN;
    o.w00 = 1.0;
    o.w01 = o.w10 = o.w11 = 0.0;
    o.sr = o.sc = 0;
    return o;
  }
  const double lim = 32.0 * kSweepMaxShift;
  const long Y = (long)nearbyint(fmax(-lim, fmin(lim, (0.0 - px) * 32.0)));   // rows
  const long X = (long)nearbyint(fmax(-lim, fmin(lim, (0.0 - py) * 32.0)));   // columns
  o.sr = (int)(Y >> 5);
  o.sc = (int)(X >> 5);
  const float step = 1.0f / 32.0f;
  const float by = (float)(Y & 31) * step, bx = (float)(X & 31) * step;
  const float ay = 1.0f - by, ax = 1.0f - bx;
  o.w00 = (double)(ay * ax);
  o.w01 = (double)(ay * bx);
  o.w10 = (double)(by * ax);
  o.w11 = (double)(by * bx);
  return o;
}

struct SweepArgs {
  int H, W, P, K, C;            // image, boxes, hypotheses, partial winners per box
  int ph, pw, halo;             // the call's largest box and the patch route's halo
  int no_pol, has_we;
  double w_dn;
  const double *gx, *gy, *q, *we;
  size_t grad_stride, field_stride;   // elements between windows
  const int* boxes;             // [P, 4]: r0, r1, c0, c1
  const int* sel;               // [B, P] or NULL
  const Hyp* hyp;               // [K]
  double* qn;                   // [B, P]
  double* cost;                 // [B, P, K] or NULL
  double* part_cost;            // [B, P, C]
  int* part_idx;                // [B, P, C]
};

__device__ __forceinline__ bool box_ok(const SweepArgs& a, int p, int* r0, int* r1, int* c0, int* c1) {
  *r0 = a.boxes[4 * p];
  *r1 = a.boxes[4 * p + 1];
  *c0 = a.boxes[4 * p + 2];
  *c1 = a.boxes[4 * p + 3];
  return *r0 >= 0 && *r0 < *r1 && *r1 <= a.H && *c0 >= 0 && *c0 < *c1 && *c1 <= a.W && *r1 - *r0 <= a.ph && *c1 - *c0 <= a.pw;
}

// max as numpy takes it: a NaN stays
__device__ __forceinline__ double nan_max(double a, double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

// (cost, index) a before b: the lower cost, the lower index on a tie; index -1 = nothing yet
__device__ __forceinline__ void take_min(double& c, int& i, double c2, int i2) {
  if (i2 >= 0 && (i < 0 || c2 < c || (c2 == c && i2 < i))) {
    c = c2;
    i = i2;
  }
}

__global__ void __launch_bounds__(kSweepBlock) eklt_qnorm(SweepArgs a) {
  __shared__ double red[kSweepBlock];
  const int p = blockIdx.x, b = blockIdx.z, t = threadIdx.x;
  int r0, r1, c0, c1;
  const bool ok = box_ok(a, p, &r0, &r1, &c0, &c1) && (!a.sel || a.sel[(size_t)b * a.P + p] != 0);
  if (!ok) {   // uniform over the workgroup
    if (t == 0) a.qn[(size_t)b * a.P + p] = 0.0;
    return;
  }
  const double* __restrict__ q = a.q + (size_t)b * a.field_stride;
  const int bw = c1 - c0, n = (r1 - r0) * bw;
  double s = 0.0;
  for (int i = t; i < n; i += kSweepBlock) {
    const double v = q[(size_t)(r0 + i / bw) * a.W + (c0 + i % bw)];
    s += v * v;
  }
  red[t] = s;
  __syncthreads();
  for (int o = kSweepBlock / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) {
    const double nrm = sqrt(red[0]);
    a.qn[(size_t)b * a.P + p] = nrm > 0.0 ? nrm : 0.0;   // 0 and NaN: not evaluated
  }
}

// the (cost, index) of the workgroup's threads -> thread 0, in a fixed tree
__device__ __forceinline__ void block_min(double* rc, int* ri, double& c, int& i) {
  const int t = threadIdx.x;
  rc[t] = c;
  ri[t] = i;
  __syncthreads();
  for (int o = kSweepBlock / 2; o > 0; o >>= 1) {
    if (t < o) {
      double cc = rc[t];
      int ii = ri[t];
      take_min(cc, ii, rc[t + o], ri[t + o]);
      rc[t] = cc;
      ri[t] = ii;
    }
    __syncthreads();
  }
  c = rc[0];
  i = ri[0];
}

__global__ void __launch_bounds__(kSweepBlock) eklt_sweep_patch(SweepArgs a) {
  extern __shared__ double lds[];
  __shared__ double rc[kSweepBlock];
  __shared__ int ri[kSweepBlock];
  const int p = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const size_t bp = (size_t)b * a.P + p;
  const double qn = a.qn[bp];
  if (!(qn > 0.0)) {   // not evaluated (uniform): no partial winner, the cost row stays as it is
    if (t == 0) {
      a.part_cost[bp * a.C + chunk] = 0.0;
      a.part_idx[bp * a.C + chunk] = -1;
    }
    return;
  }
  int r0, r1, c0, c1;
  box_ok(a, p, &r0, &r1, &c0, &c1);   // (true: qn > 0)
  const int bh = r1 - r0, bw = c1 - c0, h = a.halo;
  const int LW = a.pw + 2 * h, LH = a.ph + 2 * h;
  double* __restrict__ Gx = lds;
  double* __restrict__ Gy = Gx + (size_t)LH * LW;
  double* __restrict__ We = Gy + (size_t)LH * LW;
  double* __restrict__ Q = We + (size_t)a.ph * a.pw;
  const double* __restrict__ gx = a.gx + (size_t)b * a.grad_stride;
  const double* __restrict__ gy = a.gy + (size_t)b * a.grad_stride;
  const double* __restrict__ q = a.q + (size_t)b * a.field_stride;
  const int eh = bh + 2 * h, ew = bw + 2 * h;
  for (int i = t; i < eh * ew; i += kSweepBlock) {
    const int lr = i / ew, lc = i % ew;
    const int r = r0 - h + lr, c = c0 - h + lc;
    const bool in = r >= 0 && r < a.H && c >= 0 && c < a.W;
    Gx[lr * LW + lc] = in ? gx[(size_t)r * a.W + c] : 0.0;
    Gy[lr * LW + lc] = in ? gy[(size_t)r * a.W + c] : 0.0;
  }
  for (int i = t; i < bh * bw; i += kSweepBlock) {
    const int lr = i / bw, lc = i % bw;
    const size_t g = (size_t)(r0 + lr) * a.W + (c0 + lc);
    Q[lr * a.pw + lc] = q[g] / qn;
    if (a.has_we) We[lr * a.pw + lc] = (a.we + (size_t)b * a.field_stride)[g];
  }
  __syncthreads();

  const int k = chunk * kSweepBlock + t;
  double cost = 0.0;
  int idx = -1;
  if (k < a.K) {
    const Hyp hy = a.hyp[k];
    // |s| <= halo - 1 by the host's choice of the halo: rows lr + halo + s .. + 1 lie inside [0, bh + 2 halo)
    const int base0 = (h + hy.sr) * LW + (h + hy.sc);
    auto p0_at = [&](int lr, int lc) -> double {
      const int o = base0 + lr * LW + lc;
      const double wx = ((Gx[o] * hy.w00 + Gx[o + 1] * hy.w01) + Gx[o + LW] * hy.w10) + Gx[o + LW + 1] * hy.w11;
      const double wy = ((Gy[o] * hy.w00 + Gy[o + 1] * hy.w01) + Gy[o + LW] * hy.w10) + Gy[o + LW + 1] * hy.w11;
      double v = hy.vx * wx + hy.vy * wy;
      if (a.no_pol) v = fabs(v);
      if (a.has_we) v *= We[lr * a.pw + lc];
      return v;
    };
    double ss = 0.0;
    for (int lr = 0; lr < bh; ++lr)
      for (int lc = 0; lc < bw; ++lc) {
        const double v = p0_at(lr, lc);
        ss += v * v;
      }
    const double nrm = sqrt(ss) + 1e-4;
    double m = 0.0;
    for (int lc = 0; lc < bw; ++lc) {
      double cs = 0.0;
      for (int lr = 0; lr < bh; ++lr) cs += fabs(p0_at(lr, lc) / nrm - Q[lr * a.pw + lc]);
      m = lc == 0 ? cs : nan_max(m, cs);
    }
    cost = a.w_dn * m;
    if (a.cost) a.cost[bp * a.K + k] = cost;
    idx = cost == cost ? k : -1;
  }
  block_min(rc, ri, cost, idx);
  if (t == 0) {
    a.part_cost[bp * a.C + chunk] = cost;
    a.part_idx[bp * a.C + chunk] = idx;
  }
}

__global__ void __launch_bounds__(kSweepBlock) eklt_sweep_roi(SweepArgs a) {
  __shared__ double red[kSweepBlock];
  const int k = blockIdx.x, p = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  const size_t bp = (size_t)b * a.P + p;
  const double qn = a.qn[bp];
  if (!(qn > 0.0)) {
    if (t == 0) {
      a.part_cost[bp * a.C + k] = 0.0;
      a.part_idx[bp * a.C + k] = -1;
    }
    return;
  }
  int r0, r1, c0, c1;
  box_ok(a, p, &r0, &r1, &c0, &c1);
  const int bh = r1 - r0, bw = c1 - c0;
  const double* __restrict__ gx = a.gx + (size_t)b * a.grad_stride;
  const double* __restrict__ gy = a.gy + (size_t)b * a.grad_stride;
  const double* __restrict__ q = a.q + (size_t)b * a.field_stride;
  const double* __restrict__ we = a.has_we ? a.we + (size_t)b * a.field_stride : nullptr;
  const Hyp hy = a.hyp[k];
  const int H = a.H, W = a.W;
  auto tap = [&](const double* __restrict__ g, int r, int c) -> double {
    return (r >= 0 && r < H && c >= 0 && c < W) ? g[(size_t)r * W + c] : 0.0;
  };
  auto p0_at = [&](int r, int c) -> double {   // image coordinates of a pixel of the box
    const int sr = r + hy.sr, sc = c + hy.sc;
    const double wx = ((tap(gx, sr, sc) * hy.w00 + tap(gx, sr, sc + 1) * hy.w01) + tap(gx, sr + 1, sc) * hy.w10) + tap(gx, sr + 1, sc + 1) * hy.w11;
    const double wy = ((tap(gy, sr, sc) * hy.w00 + tap(gy, sr, sc + 1) * hy.w01) + tap(gy, sr + 1, sc) * hy.w10) + tap(gy, sr + 1, sc + 1) * hy.w11;
    double v = hy.vx * wx + hy.vy * wy;
    if (a.no_pol) v = fabs(v);
    if (we) v *= we[(size_t)r * W + c];
    return v;
  };
  const int64_t n = (int64_t)bh * bw;
  double ss = 0.0;
  for (int64_t i = t; i < n; i += kSweepBlock) {
    const double v = p0_at(r0 + (int)(i / bw), c0 + (int)(i % bw));
    ss += v * v;
  }
  red[t] = ss;
  __syncthreads();
  for (int o = kSweepBlock / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const double nrm = sqrt(red[0]) + 1e-4;
  __syncthreads();
  double m = 0.0;   // column sums are >= 0 or NaN
  for (int lc = t; lc < bw; lc += kSweepBlock) {
    double cs = 0.0;
    for (int lr = 0; lr < bh; ++lr) cs += fabs(p0_at(r0 + lr, c0 + lc) / nrm - q[(size_t)(r0 + lr) * W + (c0 + lc)] / qn);
    m = nan_max(m, cs);
  }
  red[t] = m;
  __syncthreads();
  for (int o = kSweepBlock / 2; o > 0; o >>= 1) {
    if (t < o) red[t] = nan_max(red[t], red[t + o]);
    __syncthreads();
  }
  if (t == 0) {
    const double cost = a.w_dn * red[0];
    if (a.cost) a.cost[bp * a.K + k] = cost;
    a.part_cost[bp * a.C + k] = cost;
    a.part_idx[bp * a.C + k] = cost == cost ? k : -1;
  }
}

__global__ void __launch_bounds__(kSweepBlock) eklt_argmin(int64_t n, int C, const double* __restrict__ part_cost,
                                                            const int* __restrict__ part_idx, double* __restrict__ best_cost,
                                                            int* __restrict__ best_index) {
  const int64_t i = (int64_t)blockIdx.x * kSweepBlock + threadIdx.x;
  if (i >= n) return;
  double c = 0.0;
  int k = -1;
  for (int j = 0; j < C; ++j) take_min(c, k, part_cost[i * C + j], part_idx[i * C + j]);
  best_cost[i] = k >= 0 ? c : INFINITY;
  best_index[i] = k;
}

// grid [B, 2, G]: the winner's (v_x, v_y) per box, 0 where nothing won
__global__ void __launch_bounds__(kSweepBlock) eklt_scatter(int G, int K, const int* __restrict__ best_index, const double* __restrict__ hyp,
                                                             double* __restrict__ grid) {
  const int cell = blockIdx.x * kSweepBlock + threadIdx.x;
  if (cell >= G) return;
  const size_t b = blockIdx.z;
  const int k = best_index[b * G + cell];
  const bool won = k >= 0 && k < K;
  grid[(b * 2) * G + cell] = won ? hyp[4 * (size_t)k] : 0.0;
  grid[(b * 2 + 1) * G + cell] = won ? hyp[4 * (size_t)k + 1] : 0.0;
}

__global__ void __launch_bounds__(kSweepBlock) eklt_upsample(int H, int W, int s, int kr, int kc, int gh, int gw, int off_r, int off_c,
                                                              const double* __restrict__ grid, double* __restrict__ flow) {
  const int64_t n = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * kSweepBlock + threadIdx.x;
  if (i >= n) return;
  const size_t b = blockIdx.z;
  const int r = (int)(i / W), c = (int)(i % W);
  const Tap tr = up_tap(r, off_r, s, kr, gh), tc = up_tap(c, off_c, s, kc, gw);
  const size_t G = (size_t)gh * gw;
  flow[(b * 2) * n + i] = up_eval(grid + (b * 2) * G, gw, tr, tc);
  flow[(b * 2 + 1) * n + i] = up_eval(grid + (b * 2 + 1) * G, gw, tr, tc);
}

size_t sweep_align(size_t b) { return (b + 255) & ~(size_t)255; }

size_t sweep_lds_bytes(int ph, int pw, int halo) {
  return sizeof(double) * (2 * (size_t)(ph + 2 * halo) * (size_t)(pw + 2 * halo) + 2 * (size_t)ph * (size_t)pw);
}

bool sweep_fits(int ph, int pw, int halo) {
  return ph >= 1 && pw >= 1 && halo >= 1 && ph <= 4096 && pw <= 4096 && halo <= 4096 && sweep_lds_bytes(ph, pw, halo) <= kSweepLdsBytes;
}

struct SweepLayout {
  size_t hyp, qn, part_cost, part_idx, total;
};

// C: the partial winners per box -- a chunk of 256 hypotheses each (patch route) or one hypothesis each (ROI route)
int sweep_partials(int K, bool patch) { return patch ? (K + kSweepBlock - 1) / kSweepBlock : K; }

SweepLayout sweep_layout(int nw, int P, int K, int C) {
  const size_t bp = (size_t)nw * P;
  SweepLayout L;
  size_t o = 0;
  L.hyp = o; o += sweep_align((size_t)K * sizeof(Hyp));
  L.qn = o; o += sweep_align(bp * sizeof(double));
  L.part_cost = o; o += sweep_align(bp * C * sizeof(double));
  L.part_idx = o; o += sweep_align(bp * C * sizeof(int));
  L.total = o;
  return L;
}

// the halo a table needs: max |integer shift| + 1
int sweep_halo(const double* hyp, int K) {
  int shift = 0;
  for (int k = 0; k < K; ++k) {
    const Hyp h = eklt_hypothesis(hyp + 4 * (size_t)k);
    shift = std::max(shift, std::max(std::abs(h.sr), std::abs(h.sc)));
  }
  return shift + 1;
}

}  // namespace
}  // namespace ebos

extern "C" {

int ebos_eklt_sweep_fits(int ph, int pw, int halo) { return ebos::sweep_fits(ph, pw, halo) ? 1 : 0; }

int ebos_eklt_sweep_halo(const double* hyp, int n_hyp) { return hyp && n_hyp >= 1 ? ebos::sweep_halo(hyp, n_hyp) : 0; }

size_t ebos_eklt_sweep_scratch_bytes(int n_windows, int n_boxes, int n_hyp, int route) {
  if (n_windows < 1 || n_windows > ebos::kSweepMaxWindows || n_boxes < 1 || n_hyp < 1) return 0;
  return ebos::sweep_layout(n_windows, n_boxes, n_hyp, ebos::sweep_partials(n_hyp, route == EBOS_EKLT_ROUTE_PATCH)).total;
}

int ebos_eklt_sweep_batch_f64(int n_windows, int H, int W, const double* gx, const double* gy, int64_t grad_stride, const double* q,
                              const double* we, const int* boxes, int n_boxes, int ph, int pw, const int* sel, const double* hyp,
                              int n_hyp, int flags, double w_diff_norm, int route, double* cost, double* best_cost, int* best_index,
                              void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  const char* who = "ebos_eklt_sweep_batch_f64";
  EBOS_REQUIRE(n_windows >= 1 && n_windows <= kSweepMaxWindows, "%s: %d windows", who, n_windows);
  EBOS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31), "%s: bad image size %d x %d", who, H, W);
  EBOS_REQUIRE(n_boxes >= 1 && n_hyp >= 1 && (int64_t)n_windows * n_boxes * n_hyp < ((int64_t)1 << 40), "%s: %d boxes, %d hypotheses", who,
               n_boxes, n_hyp);
  EBOS_REQUIRE(ph >= 1 && ph <= H && pw >= 1 && pw <= W, "%s: box bound %d x %d does not fit the image", who, ph, pw);
  EBOS_REQUIRE(gx && gy && q && boxes && hyp && best_cost && best_index && scratch, "%s: NULL buffer", who);
  EBOS_REQUIRE(grad_stride == 0 || grad_stride == (int64_t)H * W, "%s: grad stride is neither 0 nor H W", who);
  EBOS_REQUIRE(!(flags & EBOS_GML_EVENT_WEIGHTS) == !we, "%s: EBOS_GML_EVENT_WEIGHTS and we go together", who);
  EBOS_REQUIRE((flags & ~(EBOS_GML_NO_POLARITY | EBOS_GML_EVENT_WEIGHTS)) == 0, "%s: unknown flags %d", who, flags);
  EBOS_REQUIRE(route >= EBOS_EKLT_ROUTE_AUTO && route <= EBOS_EKLT_ROUTE_ROI, "%s: unknown route %d", who, route);
  std::vector<Hyp> table((size_t)n_hyp);
  int shift = 0;
  for (int k = 0; k < n_hyp; ++k) {
    table[k] = eklt_hypothesis(hyp + 4 * (size_t)k);
    shift = std::max(shift, std::max(std::abs(table[k].sr), std::abs(table[k].sc)));
  }
  const int halo = shift + 1;
  const bool fits = sweep_fits(ph, pw, halo);
  if (route == EBOS_EKLT_ROUTE_PATCH && !fits) {
    set_error("%s: box %d x %d with halo %d does not fit the patch route's LDS", who, ph, pw, halo);
    return EBOS_ERR_UNSUPPORTED;
  }
  const bool patch = route == EBOS_EKLT_ROUTE_PATCH || (route == EBOS_EKLT_ROUTE_AUTO && fits);
  if (!patch && n_boxes > 65535) {
    set_error("%s: %d boxes on the ROI route (at most 65535)", who, n_boxes);
    return EBOS_ERR_UNSUPPORTED;
  }
  const int C = sweep_partials(n_hyp, patch);
  if (patch && C > 65535) {
    set_error("%s: %d hypotheses on the patch route (at most %d)", who, n_hyp, 65535 * kSweepBlock);
    return EBOS_ERR_UNSUPPORTED;
  }
  const SweepLayout L = sweep_layout(n_windows, n_boxes, n_hyp, C);
  if (scratch_bytes < L.total) {
    set_error("%s: scratch too small (%zu < %zu)", who, scratch_bytes, L.total);
    return EBOS_ERR_SCRATCH;
  }
  char* s = static_cast<char*>(scratch);
  const hipStream_t st = as_stream(stream);
  // (pageable memory: the copy has left the host buffer when the call returns)
  if (hipMemcpyAsync(s + L.hyp, table.data(), (size_t)n_hyp * sizeof(Hyp), hipMemcpyHostToDevice, st) != hipSuccess) {
    set_error("%s: the hypothesis table's copy failed", who);
    return EBOS_ERR_LAUNCH;
  }
  SweepArgs a;
  a.H = H; a.W = W; a.P = n_boxes; a.K = n_hyp; a.C = C;
  a.ph = ph; a.pw = pw; a.halo = halo;
  a.no_pol = (flags & EBOS_GML_NO_POLARITY) ? 1 : 0;
  a.has_we = we ? 1 : 0;
  a.w_dn = w_diff_norm;
  a.gx = gx; a.gy = gy; a.q = q; a.we = we;
  a.grad_stride = (size_t)grad_stride;
  a.field_stride = (size_t)H * W;
  a.boxes = boxes; a.sel = sel;
  a.hyp = reinterpret_cast<const Hyp*>(s + L.hyp);
  a.qn = reinterpret_cast<double*>(s + L.qn);
  a.cost = cost;
  a.part_cost = reinterpret_cast<double*>(s + L.part_cost);
  a.part_idx = reinterpret_cast<int*>(s + L.part_idx);
  hipLaunchKernelGGL(eklt_qnorm, dim3(n_boxes, 1, n_windows), dim3(kSweepBlock), 0, st, a);
  if (patch) {
    const size_t lds = sweep_lds_bytes(ph, pw, halo);
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(eklt_sweep_patch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      set_error("%s: %zu bytes of LDS refused", who, lds);
      return EBOS_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(eklt_sweep_patch, dim3(n_boxes, C, n_windows), dim3(kSweepBlock), lds, st, a);
  } else {
    hipLaunchKernelGGL(eklt_sweep_roi, dim3(n_hyp, n_boxes, n_windows), dim3(kSweepBlock), 0, st, a);
  }
  const int64_t nbp = (int64_t)n_windows * n_boxes;
  hipLaunchKernelGGL(eklt_argmin, dim3((unsigned)((nbp + kSweepBlock - 1) / kSweepBlock)), dim3(kSweepBlock), 0, st, nbp, C, a.part_cost,
                     a.part_idx, best_cost, best_index);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

int ebos_eklt_patch_flow_batch_f64(int n_windows, int H, int W, int patch, int slide, int gh, int gw, const int* best_index,
                                   const double* hyp, int n_hyp, double* grid, double* flow, ebos_stream_t stream) {
  using namespace ebos;
  const char* who = "ebos_eklt_patch_flow_batch_f64";
  EBOS_REQUIRE(n_windows >= 1 && n_windows <= kSweepMaxWindows, "%s: %d windows", who, n_windows);
  EBOS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31), "%s: bad image size %d x %d", who, H, W);
  EBOS_REQUIRE(patch >= 1 && slide >= 1 && patch <= H && patch <= W, "%s: patch %d / slide %d do not fit %d x %d", who, patch, slide, H, W);
  // len(arange(0, L - p + s, s)) cells per axis
  EBOS_REQUIRE(gh == (H - patch + 2 * slide - 1) / slide && gw == (W - patch + 2 * slide - 1) / slide, "%s: grid %d x %d is not the patch grid",
               who, gh, gw);
  EBOS_REQUIRE(best_index && hyp && n_hyp >= 1 && grid && flow, "%s: NULL buffer", who);
  const int k = (int)floor((patch / 2.0) / slide) + 1;   // int(patch / 2 // slide) + 1
  const int off_r = (gh + 2 * k) * slide / 2 - H / 2, off_c = (gw + 2 * k) * slide / 2 - W / 2;
  EBOS_REQUIRE(off_r >= 0 && off_r + H <= (gh + 2 * k) * slide && off_c >= 0 && off_c + W <= (gw + 2 * k) * slide,
               "%s: the centre crop leaves the upsampled canvas", who);
  const hipStream_t st = as_stream(stream);
  const int G = gh * gw;
  hipLaunchKernelGGL(eklt_scatter, dim3((G + kSweepBlock - 1) / kSweepBlock, 1, n_windows), dim3(kSweepBlock), 0, st, G, n_hyp, best_index, hyp,
                     grid);
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(eklt_upsample, dim3((unsigned)((n + kSweepBlock - 1) / kSweepBlock), 1, n_windows), dim3(kSweepBlock), 0, st, H, W, slide, k,
                     k, gh, gw, off_r, off_c, grid, flow);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

}  // extern "C"
