// gml.hip -- the reference's generative BOS solver, patch_eklt_pyramid2 (src/solver/patch_eklt_pyramid2.py), in float64:
// per window a prepare step (model-image gradients, measurement, inverse-histogram weights) and, per pyramid scale, `iters`
// Adam iterations of the objective
//
//   F = up(Sobel3_replicate(x[0]) / 8),  T = up(x[1:3]),  P0 = F0 warp(gx, T) + F1 warp(gy, T)  (|P0| if no_polarity, * We M)
//   P = P0 / (|P0|_F + 1e-4) M,   L = w_dn max_c sum_r |Q M - P| + w_ig mean(|d_r(F M) winv| + |d_c(F M) winv|)
//                                   + w_fn mean_px |T M|_2
//
// `up` is the patch -> dense upsample at patch = slide = p (replicate pad 1, bilinear with align_corners=False at the integer
// factor p, centre crop), `warp` frame_utils.warp_image_forward (grid_sample, bilinear, align_corners=True, zeros; the base
// grid rounded to float32 as torch builds it), d_r / d_c torch.gradient.  Gradients are torch's: amax splits evenly among tied
// columns, abs'(0) = 0, the pxy norm's gradient is 0 where the norm is 0.
//
// One iteration = seven launches on the caller's stream, no atomics, every reduction in a fixed order:
//   gml_sobel     S = Sobel3(x0) / 8 on the [gh, gw] grid                                   (one thread per cell)
//   gml_pass_a    per pixel: F, T, warps, P0 -> P0 buffer; block partials of sum P0^2, of the image_gradient sum and of the
//                 pxy-norm sum (fixed grid-stride mapping: the partial of a pixel never depends on the launch)
//   gml_pass_b    per (16-row block, column): N = |P0| from the pass-A partials (same order in every block), D = Q M - P,
//                 partial column sums of |D|
//   gml_pass_c    one workgroup: column sums, their max, the tie set (colw[c] = w_dn / #ties on tied columns), the loss and its
//                 parts into the history, S = sum G M P0 over the tied columns
//   gml_pass_d    per pixel: dL/dP0 (direct term and the norm's), then dL/dF (through the warped gradients and the
//                 image_gradient stencil's adjoint) and dL/dT (through d warp / dT and the pxy-norm adjoint) -> dF, dT buffers
//   gml_pass_e    per grid cell: the upsample's adjoint, a gather over the pixels the cell reaches (fixed order)
//   gml_adam      per grid cell: the Sobel adjoint of dS -> dx0, then torch.optim.Adam's update (or, for the objective
//                 entry, the gradient written out)
#pragma clang fp contract(off)

#include <math.h>

#include "common.h"

namespace ebos {
namespace {

constexpr int kGmlBlock = 256;
constexpr int kGmlRowsB = 16;       // rows per pass-B block
constexpr int kGmlMaxPartA = 512;   // pass-A workgroups (at most)
constexpr int kGmlScalars = 8;      // N, S, ...

struct GmlGeom {
  int H, W, p, gh, gw, off_r, off_c;
  int xmin, xmax, ymin, ymax;       // ROI rows [xmin, xmax), columns [ymin, ymax)
  int warp, no_pol, has_we;
  int nbA;                          // pass-A workgroups
  int rbB;                          // pass-B row blocks
  double w_dn, w_ig, w_fn;          // 0 = term absent
  int order[3], n_terms;            // term indices (0 dn, 1 ig, 2 fn) in the configuration's order
};

struct GmlBufs {
  const double *gx, *gy, *q, *we, *winv;
  double *x;                        // [nd, gh, gw]
  double *S;                        // [2, gh, gw]
  double *P0;                       // [H, W]
  double *dF, *dT;                  // [2, H, W] each
  double *partA;                    // [3, nbA]
  double *colpart;                  // [rbB, W]
  double *colw;                     // [W]
  double *scal;                     // [kGmlScalars]
  double *gS, *gX;                  // [2, gh, gw] each: d/dS, d/dx[1:3]
  double *m, *v;                    // Adam state [nd, gh, gw]
};

__host__ __device__ inline int64_t gml_npix(const GmlGeom& g) { return (int64_t)g.H * g.W; }

size_t gml_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct GmlLayout {
  size_t S, P0, dF, dT, partA, colpart, colw, scal, gS, gX, m, v, total;
};

GmlLayout gml_layout(int H, int W, int G) {
  const size_t d = sizeof(double);
  const size_t hw = (size_t)H * W;
  const int rb = (H + kGmlRowsB - 1) / kGmlRowsB;
  GmlLayout L;
  size_t o = 0;
  L.S = o; o += gml_align(2 * (size_t)G * d);
  L.P0 = o; o += gml_align(hw * d);
  L.dF = o; o += gml_align(2 * hw * d);
  L.dT = o; o += gml_align(2 * hw * d);
  L.partA = o; o += gml_align(3 * (size_t)kGmlMaxPartA * d);
  L.colpart = o; o += gml_align((size_t)rb * W * d);
  L.colw = o; o += gml_align((size_t)W * d);
  L.scal = o; o += gml_align(kGmlScalars * d);
  L.gS = o; o += gml_align(2 * (size_t)G * d);
  L.gX = o; o += gml_align(2 * (size_t)G * d);
  L.m = o; o += gml_align(3 * (size_t)G * d);
  L.v = o; o += gml_align(3 * (size_t)G * d);
  L.total = o;
  return L;
}

// ---- the patch -> dense upsample: one axis -----------------------------------------------------------------------------
// upsampled index o = r + off; source coordinate max((o + 0.5) / p - 0.5, 0) on the (g + 2)-cell padded axis; padded cell i
// is grid cell clamp(i - 1, 0, g - 1).  (torch's upsample_bilinear2d, align_corners=False, scale = 1 / p.)
struct Tap {
  int c0, c1;
  double l0, l1;
};

__device__ __forceinline__ Tap up_tap(int r, int off, int p, int g) {
  const double scale = 1.0 / (double)p;
  double src = scale * ((double)(r + off) + 0.5) - 0.5;
  if (src < 0.0) src = 0.0;
  int i0 = (int)src;
  const int padded = g + 2;
  const int i1 = i0 + ((i0 < padded - 1) ? 1 : 0);
  double l1 = src - (double)i0;
  l1 = l1 < 0.0 ? 0.0 : (l1 > 1.0 ? 1.0 : l1);
  Tap t;
  t.l1 = l1;
  t.l0 = 1.0 - l1;
  t.c0 = min(max(i0 - 1, 0), g - 1);
  t.c1 = min(max(i1 - 1, 0), g - 1);
  return t;
}

__device__ __forceinline__ double up_eval(const double* __restrict__ grid, int gw, const Tap& tr, const Tap& tc) {
  const double v00 = grid[tr.c0 * gw + tc.c0], v01 = grid[tr.c0 * gw + tc.c1];
  const double v10 = grid[tr.c1 * gw + tc.c0], v11 = grid[tr.c1 * gw + tc.c1];
  return tr.l0 * (tc.l0 * v00 + tc.l1 * v01) + tr.l1 * (tc.l0 * v10 + tc.l1 * v11);
}

__device__ __forceinline__ bool in_roi(const GmlGeom& g, int r, int c) {
  return r >= g.xmin && r < g.xmax && c >= g.ymin && c < g.ymax;
}

// U_ch(r, c) = F_ch(r, c) M(r, c), the flow the image_gradient term sees.
__device__ __forceinline__ double u_at(const GmlGeom& g, const double* __restrict__ S, int ch, int r, int c) {
  const Tap tr = up_tap(r, g.off_r, g.p, g.gh), tc = up_tap(c, g.off_c, g.p, g.gw);
  const double m = in_roi(g, r, c) ? 1.0 : 0.0;
  return up_eval(S + (size_t)ch * g.gh * g.gw, g.gw, tr, tc) * m;
}

// torch.gradient of U along rows at (i, c) (spacing 1, edge_order 1) and along columns at (r, j)
__device__ __forceinline__ double grad_r(const GmlGeom& g, const double* S, int ch, int i, int c) {
  if (i == 0) return u_at(g, S, ch, 1, c) - u_at(g, S, ch, 0, c);
  if (i == g.H - 1) return u_at(g, S, ch, g.H - 1, c) - u_at(g, S, ch, g.H - 2, c);
  return (u_at(g, S, ch, i + 1, c) - u_at(g, S, ch, i - 1, c)) / 2.0;
}
__device__ __forceinline__ double grad_c(const GmlGeom& g, const double* S, int ch, int r, int j) {
  if (j == 0) return u_at(g, S, ch, r, 1) - u_at(g, S, ch, r, 0);
  if (j == g.W - 1) return u_at(g, S, ch, r, g.W - 1) - u_at(g, S, ch, r, g.W - 2);
  return (u_at(g, S, ch, r, j + 1) - u_at(g, S, ch, r, j - 1)) / 2.0;
}

__device__ __forceinline__ double sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// warp_image_forward of gx and gy at pixel (r, c) by T = (T0, T1), and the derivatives of both by T0 and T1.
struct Warped {
  double gx, gy, dgx0, dgx1, dgy0, dgy1;
};

__device__ __forceinline__ Warped warp_at(const GmlGeom& g, const double* __restrict__ gx, const double* __restrict__ gy, int r, int c,
                                          double T0, double T1) {
  const double kh = (g.H - 1) / 2.0, kw = (g.W - 1) / 2.0;
  const float cr = (float)r / (float)kh - 1.0f;   // the float32 base grid
  const float cc = (float)c / (float)kw - 1.0f;
  const double wx = (double)cr - T0 / kh;         // normalised row
  const double wy = (double)cc - T1 / kw;         // normalised column
  const double iy = (wx + 1.0) * kh;              // grid_sample unnormalise, align_corners=True
  const double ix = (wy + 1.0) * kw;
  const double fy = floor(iy), fx = floor(ix);
  const double n = iy - fy, s = 1.0 - n;          // weights of the lower / upper row
  const double w = ix - fx, e = 1.0 - w;
  const int y0 = (int)fy, x0 = (int)fx;
  double ax[4] = {0.0, 0.0, 0.0, 0.0}, ay[4] = {0.0, 0.0, 0.0, 0.0};   // nw, ne, sw, se
  const int ys[2] = {y0, y0 + 1}, xs[2] = {x0, x0 + 1};
  if (fy > -2.0 && fy < (double)g.H && fx > -2.0 && fx < (double)g.W) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int yy = ys[a], xx = xs[b];
        if (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) {
          const size_t k = (size_t)yy * g.W + xx;
          ax[a * 2 + b] = gx[k];
          ay[a * 2 + b] = gy[k];
        }
      }
  }
  Warped o;
  o.gx = s * e * ax[0] + s * w * ax[1] + n * e * ax[2] + n * w * ax[3];
  o.gy = s * e * ay[0] + s * w * ay[1] + n * e * ay[2] + n * w * ay[3];
  // d out / d iy and d out / d ix; iy = (cr - T0 / kh + 1) kh: d iy / d T0 = -1 (as torch forms it: -(g kh) / kh)
  const double gyx = (ax[2] - ax[0]) * e + (ax[3] - ax[1]) * w, gxx = (ax[1] - ax[0]) * s + (ax[3] - ax[2]) * n;
  const double gyy = (ay[2] - ay[0]) * e + (ay[3] - ay[1]) * w, gxy = (ay[1] - ay[0]) * s + (ay[3] - ay[2]) * n;
  o.dgx0 = -(gyx * kh) / kh;
  o.dgx1 = -(gxx * kw) / kw;
  o.dgy0 = -(gyy * kh) / kh;
  o.dgy1 = -(gxy * kw) / kw;
  return o;
}

// fixed-order tree sum over a 256-thread block (all threads call; result valid in thread 0)
template <int N>
__device__ __forceinline__ void block_sum(double (*sh)[kGmlBlock], double* v) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) sh[k][t] = v[k];
  __syncthreads();
  for (int s = kGmlBlock / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < N; ++k) sh[k][t] += sh[k][t + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = sh[k][0];
}

// ---- prologue: S = Sobel3(x0) / 8, replicate borders -------------------------------------------------------------------
__global__ void __launch_bounds__(kGmlBlock) gml_sobel(GmlGeom g, const double* __restrict__ x, double* __restrict__ S) {
  const int G = g.gh * g.gw;
  const int k = blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= G) return;
  const int i = k / g.gw, j = k % g.gw;
  double v[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) v[a][b] = x[min(max(i + a - 1, 0), g.gh - 1) * g.gw + min(max(j + b - 1, 0), g.gw - 1)];
  // conv2d correlation, GX = [[-1,-2,-1],[0,0,0],[1,2,1]], GY = its transpose; the kernel's taps in row-major order
  const double sx = ((((((-1.0 * v[0][0] + -2.0 * v[0][1]) + -1.0 * v[0][2]) + 0.0 * v[1][0]) + 0.0 * v[1][1]) + 0.0 * v[1][2]) +
                     1.0 * v[2][0] + 2.0 * v[2][1]) + 1.0 * v[2][2];
  const double sy = ((((((-1.0 * v[0][0] + 0.0 * v[0][1]) + 1.0 * v[0][2]) + -2.0 * v[1][0]) + 0.0 * v[1][1]) + 2.0 * v[1][2]) +
                     -1.0 * v[2][0] + 0.0 * v[2][1]) + 1.0 * v[2][2];
  S[k] = sx / 8.;
  S[G + k] = sy / 8.;
}

// ---- pass A ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGmlBlock) gml_pass_a(GmlGeom g, GmlBufs B) {
  __shared__ double sh[3][kGmlBlock];
  const int64_t n = gml_npix(g);
  const int G = g.gh * g.gw;
  double acc[3] = {0.0, 0.0, 0.0};   // sum P0^2, image_gradient sum, pxy-norm sum
  for (int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x; k < n; k += (int64_t)g.nbA * kGmlBlock) {
    const int r = (int)(k / g.W), c = (int)(k % g.W);
    const Tap tr = up_tap(r, g.off_r, g.p, g.gh), tc = up_tap(c, g.off_c, g.p, g.gw);
    const double F0 = up_eval(B.S, g.gw, tr, tc), F1 = up_eval(B.S + G, g.gw, tr, tc);
    const double M = in_roi(g, r, c) ? 1.0 : 0.0;
    double wgx, wgy, T0 = 0.0, T1 = 0.0;
    if (g.warp) {
      T0 = up_eval(B.x + G, g.gw, tr, tc);
      T1 = up_eval(B.x + 2 * (size_t)G, g.gw, tr, tc);
      const Warped w = warp_at(g, B.gx, B.gy, r, c, T0, T1);
      wgx = w.gx;
      wgy = w.gy;
    } else {
      wgx = B.gx[k];
      wgy = B.gy[k];
    }
    double P0 = F0 * wgx + F1 * wgy;
    if (g.no_pol) P0 = fabs(P0);
    if (g.has_we) P0 = P0 * (B.we[k] * M);
    B.P0[k] = P0;
    acc[0] += P0 * P0;
    if (g.w_ig != 0.0) {
      const double wi = B.winv[k];
      double s = 0.0;
      for (int ch = 0; ch < 2; ++ch) s += fabs(grad_r(g, B.S, ch, r, c) * wi) + fabs(grad_c(g, B.S, ch, r, c) * wi);
      acc[1] += s;
    }
    if (g.warp && g.w_fn != 0.0) {
      const double a = T0 * M, b = T1 * M;
      acc[2] += sqrt(a * a + b * b);
    }
  }
  block_sum<3>(sh, acc);
  if (threadIdx.x == 0) {
    B.partA[blockIdx.x] = acc[0];
    B.partA[g.nbA + blockIdx.x] = acc[1];
    B.partA[2 * g.nbA + blockIdx.x] = acc[2];
  }
}

// N = |P0|_F from the pass-A partials: the same fixed order in every caller
__device__ double gml_norm(const GmlGeom& g, const double* __restrict__ partA, double (*sh)[kGmlBlock]) {
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < g.nbA; i += kGmlBlock) v[0] += partA[i];
  block_sum<1>(sh, v);
  return sqrt(v[0]);
}

// ---- pass B ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGmlBlock) gml_pass_b(GmlGeom g, GmlBufs B) {
  __shared__ double sh[1][kGmlBlock];
  const double N = gml_norm(g, B.partA, sh);
  const double den = N + 0.0001;
  const int c = blockIdx.x * kGmlBlock + threadIdx.x;
  const int rb = blockIdx.y;
  if (c >= g.W) return;
  const int r0 = rb * kGmlRowsB, r1 = min(r0 + kGmlRowsB, g.H);
  double s = 0.0;
  for (int r = r0; r < r1; ++r) {
    const size_t k = (size_t)r * g.W + c;
    const double M = in_roi(g, r, c) ? 1.0 : 0.0;
    const double P = B.P0[k] / den * M;
    s += fabs(B.q[k] * M - P);
  }
  B.colpart[(size_t)rb * g.W + c] = s;
  if (rb == 0 && c == 0) B.scal[0] = N;
}

// ---- pass C (one workgroup) -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGmlBlock) gml_pass_c(GmlGeom g, GmlBufs B, double* __restrict__ hist_row) {
  __shared__ double sh[3][kGmlBlock];
  __shared__ double s_max;
  __shared__ int s_ties;
  const int t = threadIdx.x;
  // column sums (fixed order over row blocks) and their max
  double mx = -1.0;
  for (int c = t; c < g.W; c += kGmlBlock) {
    double s = 0.0;
    for (int rb = 0; rb < g.rbB; ++rb) s += B.colpart[(size_t)rb * g.W + c];
    B.colw[c] = s;   // the column sum, for now
    mx = fmax(mx, s);
  }
  sh[0][t] = mx;
  __syncthreads();
  for (int s = kGmlBlock / 2; s > 0; s >>= 1) {
    if (t < s) sh[0][t] = fmax(sh[0][t], sh[0][t + s]);
    __syncthreads();
  }
  if (t == 0) s_max = sh[0][0];
  __syncthreads();
  const double cmax = s_max;
  double cnt[1] = {0.0};
  for (int c = t; c < g.W; c += kGmlBlock) cnt[0] += (B.colw[c] == cmax) ? 1.0 : 0.0;
  __syncthreads();
  block_sum<1>(sh, cnt);
  if (t == 0) s_ties = (int)cnt[0];
  __syncthreads();
  const double share = g.w_dn / (double)s_ties;
  for (int c = t; c < g.W; c += kGmlBlock) B.colw[c] = (B.colw[c] == cmax) ? share : 0.0;
  // the other two terms from the pass-A partials
  double v[2] = {0.0, 0.0};
  for (int i = t; i < g.nbA; i += kGmlBlock) {
    v[0] += B.partA[g.nbA + i];
    v[1] += B.partA[2 * g.nbA + i];
  }
  __syncthreads();
  block_sum<2>(sh, v);
  const double hw = (double)gml_npix(g);
  const double term[3] = {cmax, v[0] / (2.0 * hw), v[1] / hw};
  if (t == 0 && hist_row) {
    double loss = 0.0;
    for (int i = 0; i < g.n_terms; ++i) {
      const int k = g.order[i];
      const double w = k == 0 ? g.w_dn : (k == 1 ? g.w_ig : g.w_fn);
      loss = loss + w * term[k];
    }
    hist_row[0] = loss;
    hist_row[1] = term[0];
    hist_row[2] = term[1];
    hist_row[3] = term[2];
  }
  // S = sum over the tied columns of G M P0, G = colw sign(P - Q M); the tied columns of each 256-column chunk are listed in
  // ascending order first (one thread), so that the block does not walk every column
  __shared__ int s_flag[kGmlBlock];
  __shared__ int s_list[kGmlBlock];
  __shared__ int s_nlist;
  const double den = B.scal[0] + 0.0001;
  double sacc[1] = {0.0};
  __syncthreads();
  for (int base = 0; base < g.W; base += kGmlBlock) {
    const int c = base + t;
    s_flag[t] = (c < g.W && B.colw[c] != 0.0) ? 1 : 0;
    __syncthreads();
    if (t == 0) {
      int nl = 0;
      for (int i = 0; i < kGmlBlock; ++i)
        if (s_flag[i]) s_list[nl++] = base + i;
      s_nlist = nl;
    }
    __syncthreads();
    const int nl = s_nlist;
    for (int i = 0; i < nl; ++i) {
      const int cc = s_list[i];
      const double cw = B.colw[cc];
      for (int r = t; r < g.H; r += kGmlBlock) {
        const size_t k = (size_t)r * g.W + cc;
        const double M = in_roi(g, r, cc) ? 1.0 : 0.0;
        const double P = B.P0[k] / den * M;
        sacc[0] += cw * sgn(P - B.q[k] * M) * M * B.P0[k];
      }
    }
    __syncthreads();
  }
  block_sum<1>(sh, sacc);
  if (t == 0) B.scal[1] = sacc[0];
}

// ---- pass D -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGmlBlock) gml_pass_d(GmlGeom g, GmlBufs B) {
  const int64_t n = gml_npix(g);
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= n) return;
  const int G = g.gh * g.gw;
  const int r = (int)(k / g.W), c = (int)(k % g.W);
  const Tap tr = up_tap(r, g.off_r, g.p, g.gh), tc = up_tap(c, g.off_c, g.p, g.gw);
  const double F0 = up_eval(B.S, g.gw, tr, tc), F1 = up_eval(B.S + G, g.gw, tr, tc);
  const double M = in_roi(g, r, c) ? 1.0 : 0.0;
  const double N = B.scal[0], Ssum = B.scal[1];
  const double den = N + 0.0001;
  double T0 = 0.0, T1 = 0.0;
  Warped w;
  if (g.warp) {
    T0 = up_eval(B.x + G, g.gw, tr, tc);
    T1 = up_eval(B.x + 2 * (size_t)G, g.gw, tr, tc);
    w = warp_at(g, B.gx, B.gy, r, c, T0, T1);
  } else {
    w.gx = B.gx[k];
    w.gy = B.gy[k];
    w.dgx0 = w.dgx1 = w.dgy0 = w.dgy1 = 0.0;
  }
  const double P0 = B.P0[k];
  double dP0 = 0.0;
  const double cw = B.colw[c];
  if (cw != 0.0) {
    const double P = P0 / den * M;
    dP0 = cw * sgn(P - B.q[k] * M) * M / den;
  }
  if (N > 0.0) dP0 = dP0 - Ssum / (den * den) * (P0 / N);
  if (g.has_we) dP0 = dP0 * (B.we[k] * M);
  if (g.no_pol) dP0 = dP0 * sgn(F0 * w.gx + F1 * w.gy);
  double dF0 = dP0 * w.gx, dF1 = dP0 * w.gy;
  if (g.w_ig != 0.0 && M != 0.0) {
    const double cI = g.w_ig / (2.0 * (double)n);
    double dU[2] = {0.0, 0.0};
    for (int ch = 0; ch < 2; ++ch) {
      double a = 0.0;
      // rows: gradient entries i that read U(r, c)
      if (g.H >= 2) {
        for (int i = max(r - 1, 0); i <= min(r + 1, g.H - 1); ++i) {
          double coef;
          if (i == 0) coef = (r == 1 ? 1.0 : 0.0) - (r == 0 ? 1.0 : 0.0);
          else if (i == g.H - 1) coef = (r == g.H - 1 ? 1.0 : 0.0) - (r == g.H - 2 ? 1.0 : 0.0);
          else coef = (r == i + 1 ? 0.5 : 0.0) - (r == i - 1 ? 0.5 : 0.0);
          if (coef == 0.0) continue;
          const double wi = B.winv[(size_t)i * g.W + c];
          a += coef * cI * sgn(grad_r(g, B.S, ch, i, c) * wi) * wi;
        }
      }
      if (g.W >= 2) {
        for (int j = max(c - 1, 0); j <= min(c + 1, g.W - 1); ++j) {
          double coef;
          if (j == 0) coef = (c == 1 ? 1.0 : 0.0) - (c == 0 ? 1.0 : 0.0);
          else if (j == g.W - 1) coef = (c == g.W - 1 ? 1.0 : 0.0) - (c == g.W - 2 ? 1.0 : 0.0);
          else coef = (c == j + 1 ? 0.5 : 0.0) - (c == j - 1 ? 0.5 : 0.0);
          if (coef == 0.0) continue;
          const double wi = B.winv[(size_t)r * g.W + j];
          a += coef * cI * sgn(grad_c(g, B.S, ch, r, j) * wi) * wi;
        }
      }
      dU[ch] = a;
    }
    dF0 += dU[0] * M;
    dF1 += dU[1] * M;
  }
  B.dF[k] = dF0;
  B.dF[n + k] = dF1;
  if (g.warp) {
    double dT0 = dP0 * (F0 * w.dgx0 + F1 * w.dgy0);
    double dT1 = dP0 * (F0 * w.dgx1 + F1 * w.dgy1);
    if (g.w_fn != 0.0) {
      const double a = T0 * M, b = T1 * M;
      const double nn = sqrt(a * a + b * b);
      if (nn > 0.0) {
        const double cf = g.w_fn / (double)n;
        dT0 += cf * (a / nn) * M;
        dT1 += cf * (b / nn) * M;
      }
    }
    B.dT[k] = dT0;
    B.dT[n + k] = dT1;
  }
}

// ---- pass E: the upsample's adjoint, gathered per grid cell -----------------------------------------------------------------
__device__ __forceinline__ double tap_weight(const Tap& t, int cell) {
  return (t.c0 == cell ? t.l0 : 0.0) + (t.c1 == cell ? t.l1 : 0.0);
}

// pixel range [lo, hi) along an axis whose up_tap can name grid cell `cell`
__device__ __forceinline__ void cell_range(int cell, int g, int p, int off, int L, int* lo, int* hi) {
  const int imin = cell == 0 ? 0 : cell + 1;
  const int imax = cell == g - 1 ? g + 1 : cell + 1;
  // padded cell i is read by upsampled o with source coordinate in (i - 1, i + 1): o in ((i - 0.5) p - 0.5, (i + 1.5) p - 0.5)
  const int olo = (int)floor((imin - 0.5) * p - 0.5);
  const int ohi = (int)ceil((imax + 1.5) * p - 0.5) + 1;
  *lo = max(olo - off, 0);
  *hi = min(ohi - off, L);
}

__global__ void __launch_bounds__(kGmlBlock) gml_pass_e(GmlGeom g, GmlBufs B) {
  __shared__ double sh[4][kGmlBlock];
  const int cell = blockIdx.x;
  const int gi = cell / g.gw, gj = cell % g.gw;
  const int G = g.gh * g.gw;
  const int64_t n = gml_npix(g);
  int r0, r1, c0, c1;
  cell_range(gi, g.gh, g.p, g.off_r, g.H, &r0, &r1);
  cell_range(gj, g.gw, g.p, g.off_c, g.W, &c0, &c1);
  const int nc = max(c1 - c0, 0);
  const int64_t cnt = (int64_t)max(r1 - r0, 0) * nc;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t e = threadIdx.x; e < cnt; e += kGmlBlock) {
    const int r = r0 + (int)(e / nc), c = c0 + (int)(e % nc);
    const double wr = tap_weight(up_tap(r, g.off_r, g.p, g.gh), gi);
    if (wr == 0.0) continue;
    const double wc = tap_weight(up_tap(c, g.off_c, g.p, g.gw), gj);
    if (wc == 0.0) continue;
    const size_t k = (size_t)r * g.W + c;
    const double wgt = wr * wc;
    acc[0] += wgt * B.dF[k];
    acc[1] += wgt * B.dF[n + k];
    if (g.warp) {
      acc[2] += wgt * B.dT[k];
      acc[3] += wgt * B.dT[n + k];
    }
  }
  block_sum<4>(sh, acc);
  if (threadIdx.x == 0) {
    B.gS[cell] = acc[0];
    B.gS[G + cell] = acc[1];
    B.gX[cell] = acc[2];
    B.gX[G + cell] = acc[3];
  }
}

// ---- Sobel adjoint + Adam -----------------------------------------------------------------------------------------------------
struct AdamArgs {
  double lr, beta1, beta2, eps, step_size, bc2_sqrt;
  int step;   // 0: write the gradient to `grad_out` instead of stepping
};

__global__ void __launch_bounds__(kGmlBlock) gml_adam(GmlGeom g, GmlBufs B, AdamArgs a, double* __restrict__ grad_out) {
  const int G = g.gh * g.gw;
  const int nd = g.warp ? 3 : 1;
  const int k = blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= nd * G) return;
  const int ch = k / G, cell = k % G;
  double grad;
  if (ch == 0) {
    const int u = cell / g.gw, v = cell % g.gw;
    const double KX[3][3] = {{-1.0, -2.0, -1.0}, {0.0, 0.0, 0.0}, {1.0, 2.0, 1.0}};
    const double KY[3][3] = {{-1.0, 0.0, 1.0}, {-2.0, 0.0, 2.0}, {-1.0, 0.0, 1.0}};
    double s = 0.0;
    for (int i = max(u - 1, 0); i <= min(u + 1, g.gh - 1); ++i)
      for (int aa = 0; aa < 3; ++aa) {
        if (min(max(i + aa - 1, 0), g.gh - 1) != u) continue;
        for (int j = max(v - 1, 0); j <= min(v + 1, g.gw - 1); ++j)
          for (int bb = 0; bb < 3; ++bb) {
            if (min(max(j + bb - 1, 0), g.gw - 1) != v) continue;
            const int q = i * g.gw + j;
            s += KX[aa][bb] * (B.gS[q] / 8.) + KY[aa][bb] * (B.gS[G + q] / 8.);
          }
      }
    grad = s;
  } else {
    grad = B.gX[(size_t)(ch - 1) * G + cell];
  }
  if (!a.step) {
    grad_out[k] = grad;
    return;
  }
  // torch.optim.Adam, single-tensor path: lerp, mul + addcmul, sqrt / bc2_sqrt + eps, addcdiv
  const double w1 = 1.0 - a.beta1;
  double m = B.m[k];
  m = w1 < 0.5 ? m + w1 * (grad - m) : grad - (grad - m) * (1.0 - w1);
  double v = B.v[k] * a.beta2;
  v = v + ((1.0 - a.beta2) * grad) * grad;
  B.m[k] = m;
  B.v[k] = v;
  const double denom = sqrt(v) / a.bc2_sqrt + a.eps;
  B.x[k] = B.x[k] + (-a.step_size) * (m / denom);
}

__global__ void __launch_bounds__(kGmlBlock) gml_flow_out(GmlGeom g, const double* __restrict__ S, double* __restrict__ out) {
  const int64_t n = gml_npix(g);
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= n) return;
  const int r = (int)(k / g.W), c = (int)(k % g.W);
  const Tap tr = up_tap(r, g.off_r, g.p, g.gh), tc = up_tap(c, g.off_c, g.p, g.gw);
  const double M = in_roi(g, r, c) ? 1.0 : 0.0;
  out[k] = up_eval(S, g.gw, tr, tc) * M;
  out[n + k] = up_eval(S + (size_t)g.gh * g.gw, g.gw, tr, tc) * M;
}

// ---- prepare ------------------------------------------------------------------------------------------------------------------
// cv2.Sobel(f, CV_64F, 0, 1 | 1, 0, ksize=3), BORDER_REFLECT_101, of f = frame or log(frame + 1)
__device__ __forceinline__ int reflect101(int i, int L) {
  if (L == 1) return 0;
  const int P = 2 * (L - 1);
  i %= P;
  if (i < 0) i += P;
  return i < L ? i : P - i;
}

__global__ void __launch_bounds__(kGmlBlock) gml_frame_sobel(int H, int W, const double* __restrict__ frame, int use_log,
                                                              double* __restrict__ gx, double* __restrict__ gy) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= (int64_t)H * W) return;
  const int r = (int)(k / W), c = (int)(k % W);
  double v[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double f = frame[(size_t)reflect101(r + a - 1, H) * W + reflect101(c + b - 1, W)];
      v[a][b] = use_log ? log(f + 1) : f;
    }
  gx[k] = (v[2][0] + 2.0 * v[2][1] + v[2][2]) - (v[0][0] + 2.0 * v[0][1] + v[0][2]);
  gy[k] = (v[0][2] + 2.0 * v[1][2] + v[2][2]) - (v[0][0] + 2.0 * v[1][0] + v[2][0]);
}

__global__ void __launch_bounds__(kGmlBlock) gml_hist(int64_t n, const double* __restrict__ pol, int no_pol, double* __restrict__ hist,
                                                       double* __restrict__ absh) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= n) return;
  const double h = no_pol ? pol[k] + pol[n + k] : pol[k] - pol[n + k];
  hist[k] = h;
  absh[k] = fabs(h);
}

__global__ void __launch_bounds__(kGmlBlock) gml_mul(int64_t n, const double* __restrict__ a, double* __restrict__ b) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k < n) b[k] = a[k] * b[k];
}

// one workgroup: out[0] = sqrt(sum x^2), or the moments of x (mean, population std, max) -> out[0..2]
__global__ void __launch_bounds__(kGmlBlock) gml_reduce(int64_t n, const double* __restrict__ x, int what, double* __restrict__ out) {
  __shared__ double sh[2][kGmlBlock];
  const int t = threadIdx.x;
  if (what == 0) {
    double v[1] = {0.0};
    for (int64_t k = t; k < n; k += kGmlBlock) v[0] += x[k] * x[k];
    block_sum<1>(sh, v);
    if (t == 0) out[0] = sqrt(v[0]);
    return;
  }
  double v[2] = {0.0, 0.0};
  for (int64_t k = t; k < n; k += kGmlBlock) {
    v[0] += x[k];
    v[1] = fmax(v[1], x[k]);
  }
  sh[1][t] = v[1];
  double s[1] = {v[0]};
  block_sum<1>(sh, s);
  __syncthreads();
  for (int st = kGmlBlock / 2; st > 0; st >>= 1) {
    if (t < st) sh[1][t] = fmax(sh[1][t], sh[1][t + st]);
    __syncthreads();
  }
  const double mean = s[0] / (double)n, mx = sh[1][0];
  __syncthreads();
  double d[1] = {0.0};
  for (int64_t k = t; k < n; k += kGmlBlock) {
    const double e = fabs(x[k] - mean);
    d[0] += e * e;
  }
  block_sum<1>(sh, d);
  if (t == 0) {
    out[0] = mean;
    out[1] = sqrt(d[0] / (double)n);
    out[2] = mx;
  }
}

__global__ void __launch_bounds__(kGmlBlock) gml_scale_by(int64_t n, double* __restrict__ x, const double* __restrict__ nrm) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k < n) x[k] = x[k] / nrm[0];
}

// winv = 1 - 0.95 clip(g, 0, mean + std / 2) / max(clip(...)); g >= 0, so the max of the clipped field is min(max g, mean + std / 2)
__global__ void __launch_bounds__(kGmlBlock) gml_winv(int64_t n, const double* __restrict__ gf, const double* __restrict__ mom,
                                                       double* __restrict__ winv) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= n) return;
  const double hi = mom[0] + mom[1] / 2.;
  const double mx = fmin(fmax(mom[2], 0.0), hi);
  double v = fmin(fmax(gf[k], 0.0), hi);
  v = v / mx;
  winv[k] = 1.0 - 0.95 * v;
}

__global__ void __launch_bounds__(kGmlBlock) gml_fill(int64_t n, double* __restrict__ x, double v) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k < n) x[k] = v;
}

inline int blocks_for(int64_t n) { return (int)((n + kGmlBlock - 1) / kGmlBlock); }

int grid_cells(int L, int p) { return (L + p - 1) / p; }   // len(arange(0, L - p + p, p))

int make_geom(GmlGeom* g, int H, int W, int p, int nd, int xmin, int xmax, int ymin, int ymax, int flags, const double* w,
              const int* order, int n_terms) {
  EBOS_REQUIRE(H >= 3 && W >= 3 && (int64_t)H * W < ((int64_t)1 << 31), "ebos_gml: bad image size %d x %d", H, W);
  EBOS_REQUIRE(p >= 1 && (p & (p - 1)) == 0 && p <= 4096, "ebos_gml: patch %d is not a power of two", p);
  EBOS_REQUIRE(nd == 1 || nd == 3, "ebos_gml: n_dim %d is not 1 or 3", nd);
  EBOS_REQUIRE(0 <= xmin && xmin <= xmax && xmax <= H && 0 <= ymin && ymin <= ymax && ymax <= W, "ebos_gml: bad ROI");
  EBOS_REQUIRE(n_terms >= 0 && n_terms <= 3 && w, "ebos_gml: bad cost terms");
  g->H = H;
  g->W = W;
  g->p = p;
  g->gh = grid_cells(H, p);
  g->gw = grid_cells(W, p);
  g->off_r = (g->gh + 2) * p / 2 - H / 2;
  g->off_c = (g->gw + 2) * p / 2 - W / 2;
  g->xmin = xmin;
  g->xmax = xmax;
  g->ymin = ymin;
  g->ymax = ymax;
  g->warp = nd == 3;
  g->no_pol = (flags & EBOS_GML_NO_POLARITY) != 0;
  g->has_we = (flags & EBOS_GML_EVENT_WEIGHTS) != 0;
  g->nbA = (int)std::min<int64_t>(blocks_for((int64_t)H * W), kGmlMaxPartA);
  g->rbB = (H + kGmlRowsB - 1) / kGmlRowsB;
  g->w_dn = w[0];
  g->w_ig = w[1];
  g->w_fn = w[2];
  g->n_terms = n_terms;
  for (int i = 0; i < 3; ++i) g->order[i] = i < n_terms ? order[i] : 0;
  for (int i = 0; i < n_terms; ++i) EBOS_REQUIRE(order[i] >= 0 && order[i] <= 2, "ebos_gml: bad term index %d", order[i]);
  EBOS_REQUIRE(!(g->w_fn != 0.0 && !g->warp), "ebos_gml: flow_norm_pxy needs optimize_warp");
  return EBOS_OK;
}

GmlBufs make_bufs(const GmlLayout& L, char* s, const double* gx, const double* gy, const double* q, const double* we, const double* winv,
                  double* x) {
  GmlBufs b;
  b.gx = gx;
  b.gy = gy;
  b.q = q;
  b.we = we;
  b.winv = winv;
  b.x = x;
  b.S = reinterpret_cast<double*>(s + L.S);
  b.P0 = reinterpret_cast<double*>(s + L.P0);
  b.dF = reinterpret_cast<double*>(s + L.dF);
  b.dT = reinterpret_cast<double*>(s + L.dT);
  b.partA = reinterpret_cast<double*>(s + L.partA);
  b.colpart = reinterpret_cast<double*>(s + L.colpart);
  b.colw = reinterpret_cast<double*>(s + L.colw);
  b.scal = reinterpret_cast<double*>(s + L.scal);
  b.gS = reinterpret_cast<double*>(s + L.gS);
  b.gX = reinterpret_cast<double*>(s + L.gX);
  b.m = reinterpret_cast<double*>(s + L.m);
  b.v = reinterpret_cast<double*>(s + L.v);
  return b;
}

// one objective + gradient evaluation: everything up to the adjoint of the upsample
int gml_forward_backward(const GmlGeom& g, const GmlBufs& B, double* hist_row, hipStream_t st) {
  const int G = g.gh * g.gw;
  const int64_t n = gml_npix(g);
  hipLaunchKernelGGL(gml_sobel, dim3(blocks_for(G)), dim3(kGmlBlock), 0, st, g, B.x, B.S);
  hipLaunchKernelGGL(gml_pass_a, dim3(g.nbA), dim3(kGmlBlock), 0, st, g, B);
  hipLaunchKernelGGL(gml_pass_b, dim3((g.W + kGmlBlock - 1) / kGmlBlock, g.rbB), dim3(kGmlBlock), 0, st, g, B);
  hipLaunchKernelGGL(gml_pass_c, dim3(1), dim3(kGmlBlock), 0, st, g, B, hist_row);
  hipLaunchKernelGGL(gml_pass_d, dim3(blocks_for(n)), dim3(kGmlBlock), 0, st, g, B);
  hipLaunchKernelGGL(gml_pass_e, dim3(G), dim3(kGmlBlock), 0, st, g, B);
  EBOS_CHECK_LAUNCH("ebos_gml passes");
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

size_t ebos_gml_scratch_bytes(int H, int W, int min_patch) {
  if (H < 3 || W < 3 || min_patch < 1) return 0;
  const int G = ebos::grid_cells(H, min_patch) * ebos::grid_cells(W, min_patch);
  const size_t hw = (size_t)H * W * sizeof(double);
  return std::max(ebos::gml_layout(H, W, G).total, 4 * ebos::gml_align(hw) + ebos::gml_align(8 * sizeof(double)));
}

int ebos_gml_prepare_f64(int H, int W, const double* frame, int use_log, const double* pol, int no_polarity, const double* blur_taps,
                         int blur_radius, const double* weight_taps, int weight_radius, const double* inv_taps, int inv_radius,
                         double* gx, double* gy, double* q, double* we, double* winv, void* scratch, size_t scratch_bytes,
                         ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(H >= 3 && W >= 3 && (int64_t)H * W < ((int64_t)1 << 31), "ebos_gml_prepare_f64: bad image size %d x %d", H, W);
  EBOS_REQUIRE(frame && pol && gx && gy && q && winv && scratch, "ebos_gml_prepare_f64: NULL buffer");
  EBOS_REQUIRE(!weight_taps == !we, "ebos_gml_prepare_f64: weight_taps and we go together");
  EBOS_REQUIRE(blur_radius >= 0 && weight_radius >= 0 && inv_radius >= 0, "ebos_gml_prepare_f64: negative radius");
  const int64_t n = (int64_t)H * W;
  const size_t plane = gml_align((size_t)n * sizeof(double));
  EBOS_REQUIRE(scratch_bytes >= 4 * plane + gml_align(8 * sizeof(double)), "ebos_gml_prepare_f64: scratch too small");
  char* s = static_cast<char*>(scratch);
  double* hist = reinterpret_cast<double*>(s);
  double* absh = reinterpret_cast<double*>(s + plane);
  double* t1 = reinterpret_cast<double*>(s + 2 * plane);
  double* t2 = reinterpret_cast<double*>(s + 3 * plane);
  double* sc = reinterpret_cast<double*>(s + 4 * plane);
  const hipStream_t st = as_stream(stream);
  const int nb = blocks_for(n);
  hipLaunchKernelGGL(gml_frame_sobel, dim3(nb), dim3(kGmlBlock), 0, st, H, W, frame, use_log, gx, gy);
  hipLaunchKernelGGL(gml_hist, dim3(nb), dim3(kGmlBlock), 0, st, n, pol, no_polarity, hist, absh);
  EBOS_CHECK_LAUNCH("ebos_gml_prepare_f64");
  int rc;
  // cv2.GaussianBlur: the row filter (along columns) first, then the column filter; reflect-101 = boundary 1
  if (blur_taps) {
    if ((rc = ebos_gauss1d_f64(hist, t1, H, W, 1, blur_taps, blur_radius, 1, stream)) != EBOS_OK) return rc;
    if ((rc = ebos_gauss1d_f64(t1, q, 1, H, W, blur_taps, blur_radius, 1, stream)) != EBOS_OK) return rc;
  } else {
    if (hipMemcpyAsync(q, hist, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) {
      set_error("ebos_gml_prepare_f64: copy failed");
      return EBOS_ERR_LAUNCH;
    }
  }
  if (weight_taps) {
    if ((rc = ebos_gauss1d_f64(absh, t1, H, W, 1, weight_taps, weight_radius, 1, stream)) != EBOS_OK) return rc;
    if ((rc = ebos_gauss1d_f64(t1, we, 1, H, W, weight_taps, weight_radius, 1, stream)) != EBOS_OK) return rc;
    hipLaunchKernelGGL(gml_mul, dim3(nb), dim3(kGmlBlock), 0, st, n, we, q);
  }
  hipLaunchKernelGGL(gml_reduce, dim3(1), dim3(kGmlBlock), 0, st, n, q, 0, sc);
  hipLaunchKernelGGL(gml_scale_by, dim3(nb), dim3(kGmlBlock), 0, st, n, q, sc);
  if (inv_taps) {
    // scipy gaussian_filter(|hist|, 10): axis 0, then axis 1, mode 'reflect' = boundary 0
    if ((rc = ebos_gauss1d_f64(absh, t1, 1, H, W, inv_taps, inv_radius, 0, stream)) != EBOS_OK) return rc;
    if ((rc = ebos_gauss1d_f64(t1, t2, H, W, 1, inv_taps, inv_radius, 0, stream)) != EBOS_OK) return rc;
    hipLaunchKernelGGL(gml_reduce, dim3(1), dim3(kGmlBlock), 0, st, n, t2, 1, sc + 1);
    hipLaunchKernelGGL(gml_winv, dim3(nb), dim3(kGmlBlock), 0, st, n, t2, sc + 1, winv);
  } else {
    hipLaunchKernelGGL(gml_fill, dim3(nb), dim3(kGmlBlock), 0, st, n, winv, 1.0);
  }
  EBOS_CHECK_LAUNCH("ebos_gml_prepare_f64");
  return EBOS_OK;
}

int ebos_gml_normalize_f64(int64_t n, double* q, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(n > 0 && q && scratch && scratch_bytes >= sizeof(double), "ebos_gml_normalize_f64: bad arguments");
  const hipStream_t st = as_stream(stream);
  double* sc = static_cast<double*>(scratch);
  hipLaunchKernelGGL(gml_reduce, dim3(1), dim3(kGmlBlock), 0, st, n, q, 0, sc);
  hipLaunchKernelGGL(gml_scale_by, dim3(blocks_for(n)), dim3(kGmlBlock), 0, st, n, q, sc);
  EBOS_CHECK_LAUNCH("ebos_gml_normalize_f64");
  return EBOS_OK;
}

int ebos_gml_objective_f64(int H, int W, int patch, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags, const double* weights,
                           const int* order, int n_terms, const double* gx, const double* gy, const double* q, const double* we,
                           const double* winv, const double* x, double* parts, double* grad, void* scratch, size_t scratch_bytes,
                           ebos_stream_t stream) {
  using namespace ebos;
  GmlGeom g;
  int rc = make_geom(&g, H, W, patch, n_dim, xmin, xmax, ymin, ymax, flags, weights, order, n_terms);
  if (rc != EBOS_OK) return rc;
  EBOS_REQUIRE(gx && gy && q && winv && x && parts && grad && scratch && (!g.has_we || we), "ebos_gml_objective_f64: NULL buffer");
  const int G = g.gh * g.gw;
  const GmlLayout L = gml_layout(H, W, G);
  if (scratch_bytes < L.total) {
    set_error("ebos_gml_objective_f64: scratch too small (%zu < %zu)", scratch_bytes, L.total);
    return EBOS_ERR_SCRATCH;
  }
  GmlBufs B = make_bufs(L, static_cast<char*>(scratch), gx, gy, q, we, winv, const_cast<double*>(x));
  const hipStream_t st = as_stream(stream);
  if ((rc = gml_forward_backward(g, B, parts, st)) != EBOS_OK) return rc;
  AdamArgs a = {};
  hipLaunchKernelGGL(gml_adam, dim3(blocks_for((int64_t)n_dim * G)), dim3(kGmlBlock), 0, st, g, B, a, grad);
  EBOS_CHECK_LAUNCH("ebos_gml_objective_f64");
  return EBOS_OK;
}

int ebos_gml_solve_scale_f64(int H, int W, int patch, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags, const double* weights,
                             const int* order, int n_terms, const double* gx, const double* gy, const double* q, const double* we,
                             const double* winv, double* x, int iters, double lr, double* history, double* flow_out, void* scratch,
                             size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  GmlGeom g;
  int rc = make_geom(&g, H, W, patch, n_dim, xmin, xmax, ymin, ymax, flags, weights, order, n_terms);
  if (rc != EBOS_OK) return rc;
  EBOS_REQUIRE(gx && gy && q && winv && x && scratch && (!g.has_we || we), "ebos_gml_solve_scale_f64: NULL buffer");
  EBOS_REQUIRE(iters >= 0, "ebos_gml_solve_scale_f64: iters %d < 0", iters);
  const int G = g.gh * g.gw;
  const GmlLayout L = gml_layout(H, W, G);
  if (scratch_bytes < L.total) {
    set_error("ebos_gml_solve_scale_f64: scratch too small (%zu < %zu)", scratch_bytes, L.total);
    return EBOS_ERR_SCRATCH;
  }
  GmlBufs B = make_bufs(L, static_cast<char*>(scratch), gx, gy, q, we, winv, x);
  const hipStream_t st = as_stream(stream);
  const int64_t np = (int64_t)n_dim * G;
  hipLaunchKernelGGL(gml_fill, dim3(blocks_for(np)), dim3(kGmlBlock), 0, st, np, B.m, 0.0);
  hipLaunchKernelGGL(gml_fill, dim3(blocks_for(np)), dim3(kGmlBlock), 0, st, np, B.v, 0.0);
  AdamArgs a;
  a.lr = lr;
  a.beta1 = 0.9;
  a.beta2 = 0.999;
  a.eps = 1e-8;
  a.step = 1;
  for (int it = 0; it < iters; ++it) {
    if ((rc = gml_forward_backward(g, B, history ? history + 4 * (size_t)it : nullptr, st)) != EBOS_OK) return rc;
    const double t = (double)(it + 1);
    a.step_size = lr / (1.0 - pow(a.beta1, t));
    a.bc2_sqrt = pow(1.0 - pow(a.beta2, t), 0.5);
    hipLaunchKernelGGL(gml_adam, dim3(blocks_for(np)), dim3(kGmlBlock), 0, st, g, B, a, nullptr);
    EBOS_CHECK_LAUNCH("ebos_gml_solve_scale_f64: adam");
  }
  if (flow_out) {
    hipLaunchKernelGGL(gml_sobel, dim3(blocks_for(G)), dim3(kGmlBlock), 0, st, g, B.x, B.S);
    hipLaunchKernelGGL(gml_flow_out, dim3(blocks_for(gml_npix(g))), dim3(kGmlBlock), 0, st, g, B.S, flow_out);
    EBOS_CHECK_LAUNCH("ebos_gml_solve_scale_f64: flow");
  }
  return EBOS_OK;
}

}  // extern "C"
