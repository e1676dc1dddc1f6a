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
//
// The single-scale solver, patch_eklt_dependent (src/solver/patch_eklt_dependent.py; ebos_gml_dep_*), runs the same passes on the
// ROI crop as the whole extent (M = 1, the upsample offset shifted by the crop's origin), over a grid of patch p and slide s (pad
// k = p / (2s) + 1), with the direct-velocity model as an option (F = up(x[0:2]): no Sobel), a per-cell selection that zeroes
// the gradient of cells without parameters, and pass E as one thread per cell for small slides (gml_pass_e_cell).
#pragma clang fp contract(off)

#include <math.h>

#include "common.h"
#include "gml_upsample.h"

namespace ebos {
namespace {

constexpr int kGmlBlock = 256;
constexpr int kGmlRowsB = 16;       // rows per pass-B block
constexpr int kGmlMaxPartA = 512;   // pass-A workgroups (at most)
constexpr int kGmlScalars = 8;      // N, S, ...

struct GmlGeom {
  int H, W;                         // the objective's extent: the image (pyramid) or the ROI crop (dependent)
  int s, k, gh, gw, off_r, off_c;   // slide, replicate pad (cells), grid, upsample offset of pixel (0, 0) (the crop's origin included)
  int xmin, xmax, ymin, ymax;       // ROI rows [xmin, xmax), columns [ymin, ymax) of the extent (the mask M)
  int nd, t0;                       // parameter channels; first warp channel (p_x, p_y = x[t0], x[t0 + 1])
  int vel;                          // 1: F = up(x[0:2]) (direct velocity); 0: F = up(Sobel3(x0) / 8)
  int e_cell;                       // pass E: one thread per grid cell (small slides) instead of one workgroup per cell
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
  const int* sel;                   // [gh, gw]: 0 = the cell has no parameters (its gradient is zero), NULL = every cell
};

__host__ __device__ inline int64_t gml_npix(const GmlGeom& g) { return (int64_t)g.H * g.W; }

// The window axis: every launch carries the window as gridDim.z, and window b = blockIdx.z works on its own slice of every
// per-window array.  Strides between consecutive windows, in elements; all zero for a single window.  The body of a pass sees
// only the view of its window, so window b is computed by the operations, in the order, of a single-window launch.
struct GmlWin {
  size_t grad;      // gx, gy (0: one model image for every window)
  size_t field;     // q, we, winv
  size_t x;         // the parameters [nd, gh, gw]
  size_t scr;       // the scratch slice (S ... v), in doubles
  size_t sel;       // the selection [gh, gw]
  size_t hist;      // the history rows of one window, in doubles
  size_t out;       // the flow [2, H, W] (or the gradient of the objective entries)
};

__device__ __forceinline__ GmlBufs gml_window(const GmlGeom& g, GmlBufs B, const GmlWin& w) {
  const size_t b = blockIdx.z;
  if (b == 0) {   // window 0 (a single window always): the buffers as they are; a uniform branch past ~60 scalar instructions
    if (g.vel) B.S = B.x;
    return B;
  }
  B.gx += b * w.grad;
  B.gy += b * w.grad;
  B.q += b * w.field;
  if (B.we) B.we += b * w.field;
  B.winv += b * w.field;
  B.x += b * w.x;
  const size_t o = b * w.scr;
  B.S = g.vel ? B.x : B.S + o;   // the direct-velocity model: F = up(x[0:2])
  B.P0 += o;
  B.dF += o;
  B.dT += o;
  B.partA += o;
  B.colpart += o;
  B.colw += o;
  B.scal += o;
  B.gS += o;
  B.gX += o;
  B.m += o;
  B.v += o;
  if (B.sel) B.sel += b * w.sel;
  return B;
}

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
  L.m = o; o += gml_align(4 * (size_t)G * d);
  L.v = o; o += gml_align(4 * (size_t)G * d);
  L.total = o;
  return L;
}

// ---- the patch -> dense upsample, one axis: Tap, up_tap, up_eval of gml_upsample.h

__device__ __forceinline__ bool in_roi(const GmlGeom& g, int r, int c) {
  return r >= g.xmin && r < g.xmax && c >= g.ymin && c < g.ymax;
}

// U_ch(r, c) = F_ch(r, c) M(r, c), the flow the image_gradient term sees.
__device__ __forceinline__ double u_at(const GmlGeom& g, const double* __restrict__ S, int ch, int r, int c) {
  const Tap tr = up_tap(r, g.off_r, g.s, g.k, g.gh), tc = up_tap(c, g.off_c, g.s, g.k, g.gw);
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
__global__ void __launch_bounds__(kGmlBlock) gml_sobel(GmlGeom g, GmlBufs B0, GmlWin win) {
  const GmlBufs B = gml_window(g, B0, win);
  const double* __restrict__ x = B.x;
  double* __restrict__ S = B.S;
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
__global__ void __launch_bounds__(kGmlBlock) gml_pass_a(GmlGeom g, GmlBufs B0, GmlWin win) {
  const GmlBufs B = gml_window(g, B0, win);
  __shared__ double sh[3][kGmlBlock];
  const int64_t n = gml_npix(g);
  const int G = g.gh * g.gw;
  double acc[3] = {0.0, 0.0, 0.0};   // sum P0^2, image_gradient sum, pxy-norm sum
  for (int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x; k < n; k += (int64_t)g.nbA * kGmlBlock) {
    const int r = (int)(k / g.W), c = (int)(k % g.W);
    const Tap tr = up_tap(r, g.off_r, g.s, g.k, g.gh), tc = up_tap(c, g.off_c, g.s, g.k, g.gw);
    const double F0 = up_eval(B.S, g.gw, tr, tc), F1 = up_eval(B.S + G, g.gw, tr, tc);
    const double M = in_roi(g, r, c) ? 1.0 : 0.0;
    double wgx, wgy, T0 = 0.0, T1 = 0.0;
    if (g.warp) {
      T0 = up_eval(B.x + (size_t)g.t0 * G, g.gw, tr, tc);
      T1 = up_eval(B.x + (size_t)(g.t0 + 1) * G, g.gw, tr, tc);
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
__global__ void __launch_bounds__(kGmlBlock) gml_pass_b(GmlGeom g, GmlBufs B0, GmlWin win) {
  const GmlBufs B = gml_window(g, B0, win);
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
__global__ void __launch_bounds__(kGmlBlock) gml_pass_c(GmlGeom g, GmlBufs B0, GmlWin win, double* __restrict__ hist_row) {
  const GmlBufs B = gml_window(g, B0, win);
  if (hist_row) hist_row += blockIdx.z * win.hist;
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
__global__ void __launch_bounds__(kGmlBlock) gml_pass_d(GmlGeom g, GmlBufs B0, GmlWin win) {
  const GmlBufs B = gml_window(g, B0, win);
  const int64_t n = gml_npix(g);
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= n) return;
  const int G = g.gh * g.gw;
  const int r = (int)(k / g.W), c = (int)(k % g.W);
  const Tap tr = up_tap(r, g.off_r, g.s, g.k, g.gh), tc = up_tap(c, g.off_c, g.s, g.k, g.gw);
  const double F0 = up_eval(B.S, g.gw, tr, tc), F1 = up_eval(B.S + G, g.gw, tr, tc);
  const double M = in_roi(g, r, c) ? 1.0 : 0.0;
  const double N = B.scal[0], Ssum = B.scal[1];
  const double den = N + 0.0001;
  double T0 = 0.0, T1 = 0.0;
  Warped w;
  if (g.warp) {
    T0 = up_eval(B.x + (size_t)g.t0 * G, g.gw, tr, tc);
    T1 = up_eval(B.x + (size_t)(g.t0 + 1) * G, g.gw, tr, tc);
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
__device__ __forceinline__ void cell_range(int cell, int g, int s, int k, int off, int L, int* lo, int* hi) {
  const int imin = cell == 0 ? 0 : cell + k;
  const int imax = cell == g - 1 ? g + 2 * k - 1 : cell + k;
  // padded cell i is read by upsampled o with source coordinate in (i - 1, i + 1): o in ((i - 0.5) s - 0.5, (i + 1.5) s - 0.5)
  const int olo = (int)floor((imin - 0.5) * s - 0.5);
  const int ohi = (int)ceil((imax + 1.5) * s - 0.5) + 1;
  *lo = max(olo - off, 0);
  *hi = min(ohi - off, L);
}

// the adjoint of the upsample at one cell over the pixel rectangle [r0, r1) x [c0, c1), in row-major order from element e0 with
// stride `step` (pass E's lane mapping; step 1 = one thread walks the whole rectangle)
__device__ __forceinline__ void cell_gather(const GmlGeom& g, const GmlBufs& B, int gi, int gj, int r0, int r1, int c0, int c1,
                                            int64_t e0, int step, double* acc) {
  const int64_t n = gml_npix(g);
  const int nc = max(c1 - c0, 0);
  const int64_t cnt = (int64_t)max(r1 - r0, 0) * nc;
  for (int64_t e = e0; e < cnt; e += step) {
    const int r = r0 + (int)(e / nc), c = c0 + (int)(e % nc);
    const double wr = tap_weight(up_tap(r, g.off_r, g.s, g.k, g.gh), gi);
    if (wr == 0.0) continue;
    const double wc = tap_weight(up_tap(c, g.off_c, g.s, g.k, g.gw), gj);
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
}

__global__ void __launch_bounds__(kGmlBlock) gml_pass_e(GmlGeom g, GmlBufs B0, GmlWin win) {
  const GmlBufs B = gml_window(g, B0, win);
  __shared__ double sh[4][kGmlBlock];
  const int cell = blockIdx.x;
  const int gi = cell / g.gw, gj = cell % g.gw;
  const int G = g.gh * g.gw;
  int r0, r1, c0, c1;
  cell_range(gi, g.gh, g.s, g.k, g.off_r, g.H, &r0, &r1);
  cell_range(gj, g.gw, g.s, g.k, g.off_c, g.W, &c0, &c1);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  cell_gather(g, B, gi, gj, r0, r1, c0, c1, threadIdx.x, kGmlBlock, acc);
  block_sum<4>(sh, acc);
  if (threadIdx.x == 0) {
    B.gS[cell] = acc[0];
    B.gS[G + cell] = acc[1];
    B.gX[cell] = acc[2];
    B.gX[G + cell] = acc[3];
  }
}

// small slides (a cell reaches some (2s + 3)^2 pixels): one thread per cell, its rectangle in row-major order
__global__ void __launch_bounds__(kGmlBlock) gml_pass_e_cell(GmlGeom g, GmlBufs B0, GmlWin win) {
  const GmlBufs B = gml_window(g, B0, win);
  const int G = g.gh * g.gw;
  const int cell = blockIdx.x * kGmlBlock + threadIdx.x;
  if (cell >= G) return;
  const int gi = cell / g.gw, gj = cell % g.gw;
  int r0, r1, c0, c1;
  cell_range(gi, g.gh, g.s, g.k, g.off_r, g.H, &r0, &r1);
  cell_range(gj, g.gw, g.s, g.k, g.off_c, g.W, &c0, &c1);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  cell_gather(g, B, gi, gj, r0, r1, c0, c1, 0, 1, acc);
  B.gS[cell] = acc[0];
  B.gS[G + cell] = acc[1];
  B.gX[cell] = acc[2];
  B.gX[G + cell] = acc[3];
}

// ---- Sobel adjoint + Adam -----------------------------------------------------------------------------------------------------
struct AdamArgs {
  double lr, beta1, beta2, eps, step_size, bc2_sqrt;
  int step;   // 0: write the gradient to `grad_out` instead of stepping
};

__global__ void __launch_bounds__(kGmlBlock) gml_adam(GmlGeom g, GmlBufs B0, GmlWin win, AdamArgs a, double* __restrict__ grad_out) {
  const GmlBufs B = gml_window(g, B0, win);
  const int G = g.gh * g.gw;
  const int k = blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= g.nd * G) return;
  const int ch = k / G, cell = k % G;
  double grad;
  if (g.vel && ch < 2) {
    grad = B.gS[(size_t)ch * G + cell];
  } else if (!g.vel && ch == 0) {
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
    grad = B.gX[(size_t)(ch - g.t0) * G + cell];
  }
  if (B.sel && B.sel[cell] == 0) grad = 0.0;   // no parameter: from zero state Adam leaves x at exactly 0
  if (!a.step) {
    grad_out[blockIdx.z * win.out + k] = grad;
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

__global__ void __launch_bounds__(kGmlBlock) gml_flow_out(GmlGeom g, GmlBufs B0, GmlWin win, double* __restrict__ out) {
  const double* __restrict__ S = gml_window(g, B0, win).S;
  out += blockIdx.z * win.out;
  const int64_t n = gml_npix(g);
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= n) return;
  const int r = (int)(k / g.W), c = (int)(k % g.W);
  const Tap tr = up_tap(r, g.off_r, g.s, g.k, g.gh), tc = up_tap(c, g.off_c, g.s, g.k, g.gw);
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

__global__ void __launch_bounds__(kGmlBlock) gml_frame_sobel(int H, int W, const double* __restrict__ frame, size_t frame_stride,
                                                              int use_log, double* __restrict__ gx, double* __restrict__ gy) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= (int64_t)H * W) return;
  frame += blockIdx.z * frame_stride;   // the window axis: planes of H W elements, one per window
  gx += blockIdx.z * ((size_t)H * W);
  gy += blockIdx.z * ((size_t)H * W);
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
  pol += blockIdx.z * (size_t)(2 * n);
  hist += blockIdx.z * (size_t)n;
  absh += blockIdx.z * (size_t)n;
  const double h = no_pol ? pol[k] + pol[n + k] : pol[k] - pol[n + k];
  hist[k] = h;
  absh[k] = fabs(h);
}

__global__ void __launch_bounds__(kGmlBlock) gml_mul(int64_t n, const double* __restrict__ a, double* __restrict__ b) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k < n) b[k] = a[k] * b[k];
}

// one workgroup per window: out[0] = sqrt(sum x^2), or the moments of x (mean, population std, max) -> out[0..2]
__global__ void __launch_bounds__(kGmlBlock) gml_reduce(int64_t n, const double* __restrict__ x, size_t x_stride, int what,
                                                         double* __restrict__ out, size_t out_stride) {
  __shared__ double sh[2][kGmlBlock];
  const int t = threadIdx.x;
  x += blockIdx.z * x_stride;
  out += blockIdx.z * out_stride;
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

__global__ void __launch_bounds__(kGmlBlock) gml_scale_by(int64_t n, double* __restrict__ x, size_t x_stride, const double* __restrict__ nrm,
                                                           size_t nrm_stride) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  x += blockIdx.z * x_stride;
  nrm += blockIdx.z * nrm_stride;
  if (k < n) x[k] = x[k] / nrm[0];
}

// winv = 1 - 0.95 clip(g, 0, mean + std / 2) / max(clip(...)); g >= 0, so the max of the clipped field is min(max g, mean + std / 2)
__global__ void __launch_bounds__(kGmlBlock) gml_winv(int64_t n, const double* __restrict__ gf, const double* __restrict__ mom,
                                                       size_t mom_stride, double* __restrict__ winv) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= n) return;
  gf += blockIdx.z * (size_t)n;
  winv += blockIdx.z * (size_t)n;
  mom += blockIdx.z * mom_stride;
  const double hi = mom[0] + mom[1] / 2.;
  const double mx = fmin(fmax(mom[2], 0.0), hi);
  double v = fmin(fmax(gf[k], 0.0), hi);
  v = v / mx;
  winv[k] = 1.0 - 0.95 * v;
}

__global__ void __launch_bounds__(kGmlBlock) gml_fill(int64_t n, double* __restrict__ x, size_t x_stride, double v) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k < n) x[blockIdx.z * x_stride + k] = v;
}

inline int blocks_for(int64_t n) { return (int)((n + kGmlBlock - 1) / kGmlBlock); }

int grid_cells(int L, int p) { return (L + p - 1) / p; }   // len(arange(0, L - p + p, p))

// the parts of the geometry both solvers share: extent, ROI mask, channels, flags and cost terms
int make_geom_common(GmlGeom* g, int H, int W, int nd, int vel, int xmin, int xmax, int ymin, int ymax, int flags, const double* w,
                     const int* order, int n_terms) {
  EBOS_REQUIRE(H >= 3 && W >= 3 && (int64_t)H * W < ((int64_t)1 << 31), "ebos_gml: bad image size %d x %d", H, W);
  EBOS_REQUIRE(vel ? (nd == 2 || nd == 4) : (nd == 1 || nd == 3), "ebos_gml: n_dim %d does not fit the model", nd);
  EBOS_REQUIRE(0 <= xmin && xmin <= xmax && xmax <= H && 0 <= ymin && ymin <= ymax && ymax <= W, "ebos_gml: bad ROI");
  EBOS_REQUIRE(n_terms >= 0 && n_terms <= 3 && w, "ebos_gml: bad cost terms");
  g->H = H;
  g->W = W;
  g->xmin = xmin;
  g->xmax = xmax;
  g->ymin = ymin;
  g->ymax = ymax;
  g->nd = nd;
  g->vel = vel;
  g->t0 = nd - 2;
  g->e_cell = 0;
  g->warp = vel ? nd == 4 : nd == 3;
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

// the pyramid: patch = slide = p (a power of two), pad 1, the whole image with the ROI as a mask
int make_geom(GmlGeom* g, int H, int W, int p, int nd, int xmin, int xmax, int ymin, int ymax, int flags, const double* w,
              const int* order, int n_terms) {
  EBOS_REQUIRE(p >= 1 && (p & (p - 1)) == 0 && p <= 4096, "ebos_gml: patch %d is not a power of two", p);
  int rc = make_geom_common(g, H, W, nd, 0, xmin, xmax, ymin, ymax, flags, w, order, n_terms);
  if (rc != EBOS_OK) return rc;
  g->s = p;
  g->k = 1;
  g->gh = grid_cells(H, p);
  g->gw = grid_cells(W, p);
  g->off_r = (g->gh + 2) * p / 2 - H / 2;
  g->off_c = (g->gw + 2) * p / 2 - W / 2;
  return EBOS_OK;
}

// ---- patch_eklt_dependent: patch p, slide s, the objective on the ROI crop ------------------------------------------------------
// Grid len(arange(0, L - p + s, s)) per axis, pad k = int(p / 2 // s) + 1, upsample to (g + 2k) s, centre crop at
// h1 = (g + 2k) s // 2 - L // 2 (prepare_patch, interpolate_dense_flow_from_patch_tensor).
struct DepAxis {
  int g, k, off;
};

int dep_axis(int L, int p, int s, DepAxis* a) {
  EBOS_REQUIRE(p >= 1 && s >= 1 && p <= L && s <= 4096 && p <= 4096, "ebos_gml_dep: patch %d / slide %d do not fit %d", p, s, L);
  a->g = (L - p + s + s - 1) / s;
  a->k = p / (2 * s) + 1;
  const int up = (a->g + 2 * a->k) * s;
  a->off = up / 2 - L / 2;
  EBOS_REQUIRE(a->off >= 0 && a->off + L <= up, "ebos_gml_dep: the centre crop leaves the upsampled canvas (%d of %d)", L, up);
  return EBOS_OK;
}

// the objective's geometry: the crop [xmin, xmax) x [ymin, ymax) is the whole extent (M = 1), offsets shifted by its origin
int make_dep_geom(GmlGeom* g, int H, int W, int p, int s, int nd, int xmin, int xmax, int ymin, int ymax, int flags, const double* w,
                  const int* order, int n_terms) {
  EBOS_REQUIRE(0 <= xmin && xmin <= xmax && xmax <= H && 0 <= ymin && ymin <= ymax && ymax <= W, "ebos_gml_dep: bad ROI");
  DepAxis ar, ac;
  int rc;
  if ((rc = dep_axis(H, p, s, &ar)) != EBOS_OK || (rc = dep_axis(W, p, s, &ac)) != EBOS_OK) return rc;
  const int h = xmax - xmin, wd = ymax - ymin;
  rc = make_geom_common(g, h, wd, nd, (flags & EBOS_GML_VELOCITY) != 0, 0, h, 0, wd, flags, w, order, n_terms);
  if (rc != EBOS_OK) return rc;
  g->s = s;
  g->k = ar.k;   // ar.k == ac.k: one patch and slide for both axes
  g->gh = ar.g;
  g->gw = ac.g;
  g->off_r = ar.off + xmin;
  g->off_c = ac.off + ymin;
  g->e_cell = s <= 8;
  return EBOS_OK;
}

// the output's geometry: the full image, unmasked
GmlGeom dep_out_geom(const GmlGeom& g, int H, int W, int xmin, int ymin) {
  GmlGeom o = g;
  o.H = H;
  o.W = W;
  o.xmin = 0;
  o.xmax = H;
  o.ymin = 0;
  o.ymax = W;
  o.off_r = g.off_r - xmin;
  o.off_c = g.off_c - ymin;
  return o;
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
  b.sel = nullptr;
  return b;
}

// one objective + gradient evaluation: everything up to the adjoint of the upsample
// (`nw` windows per launch: the grid's z extent; `hist_row` is window 0's row)
int gml_forward_backward(const GmlGeom& g, const GmlBufs& B, const GmlWin& win, int nw, double* hist_row, hipStream_t st) {
  const int G = g.gh * g.gw;
  const int64_t n = gml_npix(g);
  if (!g.vel) hipLaunchKernelGGL(gml_sobel, dim3(blocks_for(G), 1, nw), dim3(kGmlBlock), 0, st, g, B, win);
  hipLaunchKernelGGL(gml_pass_a, dim3(g.nbA, 1, nw), dim3(kGmlBlock), 0, st, g, B, win);
  hipLaunchKernelGGL(gml_pass_b, dim3((g.W + kGmlBlock - 1) / kGmlBlock, g.rbB, nw), dim3(kGmlBlock), 0, st, g, B, win);
  hipLaunchKernelGGL(gml_pass_c, dim3(1, 1, nw), dim3(kGmlBlock), 0, st, g, B, win, hist_row);
  hipLaunchKernelGGL(gml_pass_d, dim3(blocks_for(n), 1, nw), dim3(kGmlBlock), 0, st, g, B, win);
  if (g.e_cell)
    hipLaunchKernelGGL(gml_pass_e_cell, dim3(blocks_for(G), 1, nw), dim3(kGmlBlock), 0, st, g, B, win);
  else
    hipLaunchKernelGGL(gml_pass_e, dim3(G, 1, nw), dim3(kGmlBlock), 0, st, g, B, win);
  EBOS_CHECK_LAUNCH("ebos_gml passes");
  return EBOS_OK;
}

constexpr int kGmlMaxWindows = 65535;   // gridDim.z

// `iters` Adam steps on every window's x in place (fresh state), then the flow of each window over the geometry `o`
int gml_adam_loop(const GmlGeom& g, const GmlGeom& o, const GmlBufs& B, const GmlWin& win, int nw, int iters, double lr, double* history,
                  double* flow_out, hipStream_t st) {
  const int G = g.gh * g.gw;
  const int64_t np = (int64_t)g.nd * G;
  hipLaunchKernelGGL(gml_fill, dim3(blocks_for(np), 1, nw), dim3(kGmlBlock), 0, st, np, B.m, win.scr, 0.0);
  hipLaunchKernelGGL(gml_fill, dim3(blocks_for(np), 1, nw), dim3(kGmlBlock), 0, st, np, B.v, win.scr, 0.0);
  AdamArgs a;
  a.lr = lr;
  a.beta1 = 0.9;
  a.beta2 = 0.999;
  a.eps = 1e-8;
  a.step = 1;
  int rc;
  for (int it = 0; it < iters; ++it) {
    if ((rc = gml_forward_backward(g, B, win, nw, history ? history + 4 * (size_t)it : nullptr, st)) != EBOS_OK) return rc;
    const double t = (double)(it + 1);
    a.step_size = lr / (1.0 - pow(a.beta1, t));
    a.bc2_sqrt = pow(1.0 - pow(a.beta2, t), 0.5);
    hipLaunchKernelGGL(gml_adam, dim3(blocks_for(np), 1, nw), dim3(kGmlBlock), 0, st, g, B, win, a, nullptr);
    EBOS_CHECK_LAUNCH("ebos_gml: adam");
  }
  if (flow_out) {
    if (!g.vel) hipLaunchKernelGGL(gml_sobel, dim3(blocks_for(G), 1, nw), dim3(kGmlBlock), 0, st, o, B, win);
    hipLaunchKernelGGL(gml_flow_out, dim3(blocks_for(gml_npix(o)), 1, nw), dim3(kGmlBlock), 0, st, o, B, win, flow_out);
    EBOS_CHECK_LAUNCH("ebos_gml: flow");
  }
  return EBOS_OK;
}

// ---- patch_eklt_dependent: the crop, the selection, the initial parameters ---------------------------------------------------
// dst[h, w] = src[xmin + r, ymin + c] of a [., W] plane
__global__ void __launch_bounds__(kGmlBlock) gml_crop(int W, int xmin, int ymin, int h, int w, const double* __restrict__ src,
                                                       size_t src_stride, double* __restrict__ dst, size_t dst_stride) {
  const int64_t k = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (k >= (int64_t)h * w) return;
  src += blockIdx.z * src_stride;
  dst += blockIdx.z * dst_stride;
  const int r = (int)(k / w), c = (int)(k % w);
  dst[k] = src[(size_t)(xmin + r) * W + (ymin + c)];
}

// events [n, 4] (x = row, y = column, t, p) binned by (floor(x), floor(y)) into the (hc + 1) x (wc + 1) count canvas, offset by
// one row and one column (row 0 and column 0 stay 0 for the summed-area table); events off the canvas are not counted.  With
// `offsets` [windows + 1], window b = blockIdx.z owns events [offsets[b], offsets[b + 1]) of the concatenated array.
__global__ void __launch_bounds__(kGmlBlock) gml_count_events(int64_t n, const int64_t* __restrict__ offsets,
                                                               const double* __restrict__ ev, int hc, int wc, int* __restrict__ cnt,
                                                               size_t cnt_stride) {
  const int64_t i = (int64_t)blockIdx.x * kGmlBlock + threadIdx.x;
  if (offsets) {
    ev += 4 * offsets[blockIdx.z];
    n = offsets[blockIdx.z + 1] - offsets[blockIdx.z];
  }
  cnt += blockIdx.z * cnt_stride;
  if (i >= n) return;
  const double fx = floor(ev[4 * i]), fy = floor(ev[4 * i + 1]);
  if (!(fx >= 0.0 && fx < (double)hc && fy >= 0.0 && fy < (double)wc)) return;
  atomicAdd(cnt + (size_t)((int)fx + 1) * (wc + 1) + ((int)fy + 1), 1);   // integer counts: the same in any order
}

// summed-area table in place: prefix sums along each row, then along each column (one thread per row / column)
__global__ void __launch_bounds__(kGmlBlock) gml_scan_rows(int hc, int wc, int* __restrict__ cnt, size_t cnt_stride) {
  const int r = blockIdx.x * kGmlBlock + threadIdx.x + 1;
  if (r > hc) return;
  cnt += blockIdx.z * cnt_stride;
  int* row = cnt + (size_t)r * (wc + 1);
  for (int c = 1; c <= wc; ++c) row[c] += row[c - 1];
}

__global__ void __launch_bounds__(kGmlBlock) gml_scan_cols(int hc, int wc, int* __restrict__ cnt, size_t cnt_stride) {
  const int c = blockIdx.x * kGmlBlock + threadIdx.x + 1;
  if (c > wc) return;
  cnt += blockIdx.z * cnt_stride;
  for (int r = 1; r <= hc; ++r) cnt[(size_t)r * (wc + 1) + c] += cnt[(size_t)(r - 1) * (wc + 1) + c];
}

// flag[cell] = the cell's centre lies in the ROI (row_box / col_box [g, 3]: box start, box end, in-ROI) and, when thresholding,
// its event box [x0, x1) x [y0, y1) holds more than `thres` events
__global__ void __launch_bounds__(kGmlBlock) gml_select(int gh, int gw, const int* __restrict__ row_box, const int* __restrict__ col_box,
                                                         const int* __restrict__ sat, size_t sat_stride, int hc, int wc,
                                                         int thresholding, double thres, int* __restrict__ flag) {
  const int cell = blockIdx.x * kGmlBlock + threadIdx.x;
  if (cell >= gh * gw) return;
  if (sat) sat += blockIdx.z * sat_stride;
  flag += blockIdx.z * (size_t)(gh * gw);
  const int i = cell / gw, j = cell % gw;
  int ok = row_box[3 * i + 2] && col_box[3 * j + 2];
  if (ok && thresholding) {
    const int x0 = min(max(row_box[3 * i], 0), hc), x1 = min(max(row_box[3 * i + 1], x0), hc);
    const int y0 = min(max(col_box[3 * j], 0), wc), y1 = min(max(col_box[3 * j + 1], y0), wc);
    const int ld = wc + 1;
    const int c = sat[(size_t)x1 * ld + y1] - sat[(size_t)x0 * ld + y1] - sat[(size_t)x1 * ld + y0] + sat[(size_t)x0 * ld + y0];
    ok = (double)c > thres;
  }
  flag[cell] = ok;
}

// one workgroup per window: sel[cell] = 1 + the cell's rank among the selected cells in row-major order (0 = not selected); count[0] = their
// number.  A block-wide inclusive scan per 256-cell chunk.
__global__ void __launch_bounds__(kGmlBlock) gml_rank(int G, int* __restrict__ sel, int* __restrict__ count) {
  __shared__ int sh[kGmlBlock];
  const int t = threadIdx.x;
  sel += blockIdx.z * (size_t)G;
  count += blockIdx.z;
  int base = 0;
  for (int c0 = 0; c0 < G; c0 += kGmlBlock) {
    const int cell = c0 + t;
    const int f = cell < G ? (sel[cell] != 0) : 0;
    sh[t] = f;
    __syncthreads();
    for (int o = 1; o < kGmlBlock; o <<= 1) {
      const int v = t >= o ? sh[t - o] : 0;
      __syncthreads();
      sh[t] += v;
      __syncthreads();
    }
    if (cell < G) sel[cell] = f ? base + sh[t] : 0;
    base += sh[kGmlBlock - 1];
    __syncthreads();
  }
  if (t == 0) count[0] = base;
}

// x [nd, gh, gw] = 0, and x[0] = draws[rank] on the selected cells when draws is not NULL (the Poisson model's potentials)
__global__ void __launch_bounds__(kGmlBlock) gml_dep_init(int G, int nd, const int* __restrict__ sel, const double* __restrict__ draws,
                                                           double* __restrict__ x) {
  const int cell = blockIdx.x * kGmlBlock + threadIdx.x;
  if (cell >= G) return;
  sel += blockIdx.z * (size_t)G;   // per window: sel [G], draws [G] (the first `count` are used), x [nd, G]
  if (draws) draws += blockIdx.z * (size_t)G;
  x += blockIdx.z * (size_t)nd * G;
  for (int ch = 0; ch < nd; ++ch) x[(size_t)ch * G + cell] = 0.0;
  if (draws && sel[cell] != 0) x[cell] = draws[sel[cell] - 1];
}

// scratch of the dependent solver: the five crop planes, then the iteration layout
struct DepLayout {
  size_t gx, gy, q, we, winv, iter, total;
  GmlLayout L;
};

DepLayout dep_layout(int h, int w, int G) {
  const size_t plane = gml_align((size_t)h * w * sizeof(double));
  DepLayout D;
  D.gx = 0;
  D.gy = plane;
  D.q = 2 * plane;
  D.we = 3 * plane;
  D.winv = 4 * plane;
  D.iter = 5 * plane;
  D.L = gml_layout(h, w, G);
  D.total = D.iter + D.L.total;
  return D;
}

// crop the five fields into the scratch and divide the cropped measurement by its own norm; -> the iteration buffers
// (window 0's; the others follow at `scr` doubles.  `src_win`: the strides of the full-image fields)
int dep_bufs(const GmlGeom& g, int W, int xmin, int ymin, const DepLayout& D, char* s, const double* gx, const double* gy, const double* q,
             const double* we, const double* winv, double* x, const int* sel, const GmlWin& src_win, size_t scr, int nw, hipStream_t st,
             GmlBufs* out) {
  const int64_t n = gml_npix(g);
  const int nb = blocks_for(n);
  const size_t ss[5] = {src_win.grad, src_win.grad, src_win.field, src_win.field, src_win.field};
  double* c[5] = {reinterpret_cast<double*>(s + D.gx), reinterpret_cast<double*>(s + D.gy), reinterpret_cast<double*>(s + D.q),
                  reinterpret_cast<double*>(s + D.we), reinterpret_cast<double*>(s + D.winv)};
  const double* src[5] = {gx, gy, q, we, winv};
  for (int i = 0; i < 5; ++i)
    if (src[i])
      hipLaunchKernelGGL(gml_crop, dim3(nb, 1, nw), dim3(kGmlBlock), 0, st, W, xmin, ymin, g.H, g.W, src[i], ss[i], c[i], scr);
  GmlBufs B = make_bufs(D.L, s + D.iter, c[0], c[1], c[2], we ? c[3] : nullptr, c[4], x);
  hipLaunchKernelGGL(gml_reduce, dim3(1, 1, nw), dim3(kGmlBlock), 0, st, n, c[2], scr, 0, B.scal + 2, scr);
  hipLaunchKernelGGL(gml_scale_by, dim3(nb, 1, nw), dim3(kGmlBlock), 0, st, n, c[2], scr, B.scal + 2, scr);
  EBOS_CHECK_LAUNCH("ebos_gml_dep: crop");
  B.sel = sel;
  *out = B;
  return EBOS_OK;
}


bool gml_windows_ok(int nw) { return nw >= 1 && nw <= kGmlMaxWindows; }

// a batch's scratch: window b's slice starts at b * stride bytes; a slice holds `need` bytes and keeps the 256-byte alignment
int gml_check_slices(const char* who, int nw, size_t need, size_t stride, size_t bytes) {
  if (nw > 1 && (stride % 256 != 0 || stride < need)) {
    set_error("%s: scratch stride %zu is not a multiple of 256 or is below a window's %zu bytes", who, stride, need);
    return EBOS_ERR_SCRATCH;
  }
  if (bytes < (size_t)(nw - 1) * stride + need) {
    set_error("%s: scratch too small (%zu < %zu)", who, bytes, (size_t)(nw - 1) * stride + need);
    return EBOS_ERR_SCRATCH;
  }
  return EBOS_OK;
}

// prepare of `nw` windows: every field is [nw, H, W] contiguous (the frame: stride 0 = one model image, whose gradients are
// formed once), and so are the four work planes in the scratch, so that one separable-filter call covers the batch
int gml_prepare(int nw, int H, int W, const double* frame, size_t frame_stride, int use_log, const double* pol, int no_polarity,
                const double* blur_taps, int blur_radius, const double* weight_taps, int weight_radius, const double* inv_taps,
                int inv_radius, double* gx, double* gy, double* q, double* we, double* winv, void* scratch, size_t scratch_bytes,
                ebos_stream_t stream) {
  EBOS_REQUIRE(gml_windows_ok(nw), "ebos_gml_prepare: %d windows", nw);
  EBOS_REQUIRE(H >= 3 && W >= 3 && (int64_t)H * W < ((int64_t)1 << 31), "ebos_gml_prepare_f64: bad image size %d x %d", H, W);
  EBOS_REQUIRE(frame && pol && gx && gy && q && winv && scratch, "ebos_gml_prepare_f64: NULL buffer");
  EBOS_REQUIRE(!weight_taps == !we, "ebos_gml_prepare_f64: weight_taps and we go together");
  EBOS_REQUIRE(blur_radius >= 0 && weight_radius >= 0 && inv_radius >= 0, "ebos_gml_prepare_f64: negative radius");
  EBOS_REQUIRE(frame_stride == 0 || frame_stride == (size_t)H * W, "ebos_gml_prepare_f64: frame stride is neither 0 nor H W");
  const int64_t n = (int64_t)H * W;
  const size_t plane = gml_align((size_t)nw * n * sizeof(double));
  EBOS_REQUIRE(scratch_bytes >= 4 * plane + gml_align((size_t)nw * 8 * sizeof(double)), "ebos_gml_prepare_f64: scratch too small");
  char* s = static_cast<char*>(scratch);
  double* hist = reinterpret_cast<double*>(s);
  double* absh = reinterpret_cast<double*>(s + plane);
  double* t1 = reinterpret_cast<double*>(s + 2 * plane);
  double* t2 = reinterpret_cast<double*>(s + 3 * plane);
  double* sc = reinterpret_cast<double*>(s + 4 * plane);   // [nw, 8]
  const hipStream_t st = as_stream(stream);
  const int nb = blocks_for(n);
  const int nbw = blocks_for(n * nw);
  const int64_t R = (int64_t)nw * H;   // rows of the batch
  hipLaunchKernelGGL(gml_frame_sobel, dim3(nb, 1, frame_stride ? nw : 1), dim3(kGmlBlock), 0, st, H, W, frame, frame_stride, use_log, gx,
                     gy);
  hipLaunchKernelGGL(gml_hist, dim3(nb, 1, nw), dim3(kGmlBlock), 0, st, n, pol, no_polarity, hist, absh);
  EBOS_CHECK_LAUNCH("ebos_gml_prepare_f64");
  int rc;
  // cv2.GaussianBlur: the row filter (along columns) first, then the column filter; reflect-101 = boundary 1
  if (blur_taps) {
    if ((rc = ebos_gauss1d_f64(hist, t1, R, W, 1, blur_taps, blur_radius, 1, stream)) != EBOS_OK) return rc;
    if ((rc = ebos_gauss1d_f64(t1, q, nw, H, W, blur_taps, blur_radius, 1, stream)) != EBOS_OK) return rc;
  } else {
    if (hipMemcpyAsync(q, hist, (size_t)nw * n * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) {
      set_error("ebos_gml_prepare_f64: copy failed");
      return EBOS_ERR_LAUNCH;
    }
  }
  if (weight_taps) {
    if ((rc = ebos_gauss1d_f64(absh, t1, R, W, 1, weight_taps, weight_radius, 1, stream)) != EBOS_OK) return rc;
    if ((rc = ebos_gauss1d_f64(t1, we, nw, H, W, weight_taps, weight_radius, 1, stream)) != EBOS_OK) return rc;
    hipLaunchKernelGGL(gml_mul, dim3(nbw), dim3(kGmlBlock), 0, st, n * nw, we, q);
  }
  hipLaunchKernelGGL(gml_reduce, dim3(1, 1, nw), dim3(kGmlBlock), 0, st, n, q, (size_t)n, 0, sc, (size_t)8);
  hipLaunchKernelGGL(gml_scale_by, dim3(nb, 1, nw), dim3(kGmlBlock), 0, st, n, q, (size_t)n, sc, (size_t)8);
  if (inv_taps) {
    // scipy gaussian_filter(|hist|, 10): axis 0, then axis 1, mode 'reflect' = boundary 0
    if ((rc = ebos_gauss1d_f64(absh, t1, nw, H, W, inv_taps, inv_radius, 0, stream)) != EBOS_OK) return rc;
    if ((rc = ebos_gauss1d_f64(t1, t2, R, W, 1, inv_taps, inv_radius, 0, stream)) != EBOS_OK) return rc;
    hipLaunchKernelGGL(gml_reduce, dim3(1, 1, nw), dim3(kGmlBlock), 0, st, n, t2, (size_t)n, 1, sc + 1, (size_t)8);
    hipLaunchKernelGGL(gml_winv, dim3(nb, 1, nw), dim3(kGmlBlock), 0, st, n, t2, sc + 1, (size_t)8, winv);
  } else {
    hipLaunchKernelGGL(gml_fill, dim3(nbw), dim3(kGmlBlock), 0, st, n * nw, winv, (size_t)0, 1.0);
  }
  EBOS_CHECK_LAUNCH("ebos_gml_prepare_f64");
  return EBOS_OK;
}

int gml_normalize(int nw, int64_t n, double* q, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(gml_windows_ok(nw) && n > 0 && q && scratch && scratch_bytes >= (size_t)nw * sizeof(double),
               "ebos_gml_normalize_f64: bad arguments");
  const hipStream_t st = as_stream(stream);
  double* sc = static_cast<double*>(scratch);   // [nw]
  hipLaunchKernelGGL(gml_reduce, dim3(1, 1, nw), dim3(kGmlBlock), 0, st, n, q, (size_t)n, 0, sc, (size_t)1);
  hipLaunchKernelGGL(gml_scale_by, dim3(blocks_for(n), 1, nw), dim3(kGmlBlock), 0, st, n, q, (size_t)n, sc, (size_t)1);
  EBOS_CHECK_LAUNCH("ebos_gml_normalize_f64");
  return EBOS_OK;
}

// one pyramid scale of `nw` windows: fields [nw, H, W] (gx, gy: stride `grad_stride`, 0 or H W), x [nw, n_dim, gh, gw],
// history rows `history_stride` doubles apart, flow [nw, 2, H, W]
int gml_solve_scale(int nw, int H, int W, int patch, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags, const double* weights,
                    const int* order, int n_terms, const double* gx, const double* gy, size_t grad_stride, const double* q,
                    const double* we, const double* winv, double* x, int iters, double lr, double* history, size_t history_stride,
                    double* flow_out, void* scratch, size_t scratch_stride, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(gml_windows_ok(nw), "ebos_gml_solve_scale: %d windows", nw);
  GmlGeom g;
  int rc = make_geom(&g, H, W, patch, n_dim, xmin, xmax, ymin, ymax, flags, weights, order, n_terms);
  if (rc != EBOS_OK) return rc;
  EBOS_REQUIRE(gx && gy && q && winv && x && scratch && (!g.has_we || we), "ebos_gml_solve_scale_f64: NULL buffer");
  EBOS_REQUIRE(iters >= 0, "ebos_gml_solve_scale_f64: iters %d < 0", iters);
  EBOS_REQUIRE(grad_stride == 0 || grad_stride == (size_t)H * W, "ebos_gml_solve_scale: gradient stride is neither 0 nor H W");
  const int G = g.gh * g.gw;
  const GmlLayout L = gml_layout(H, W, G);
  if ((rc = gml_check_slices("ebos_gml_solve_scale_f64", nw, L.total, scratch_stride, scratch_bytes)) != EBOS_OK) return rc;
  GmlBufs B = make_bufs(L, static_cast<char*>(scratch), gx, gy, q, we, winv, x);
  GmlWin win = {};
  if (nw > 1) {
    win.grad = grad_stride;
    win.field = (size_t)H * W;
    win.x = (size_t)n_dim * G;
    win.scr = scratch_stride / sizeof(double);
    win.hist = history_stride;
    win.out = 2 * (size_t)H * W;
  }
  return gml_adam_loop(g, g, B, win, nw, iters, lr, history, flow_out, as_stream(stream));
}

int gml_dep_select(int nw, int H, int W, int patch, int slide, const int* row_box, const int* col_box, const double* events,
                   int64_t n_events, const int64_t* offsets, int canvas_h, int canvas_w, int thresholding, double event_thres, int* sel,
                   int* count, void* scratch, size_t scratch_stride, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(gml_windows_ok(nw), "ebos_gml_dep_select: %d windows", nw);
  DepAxis ar, ac;
  int rc;
  EBOS_REQUIRE(H >= 3 && W >= 3, "ebos_gml_dep_select: bad image size %d x %d", H, W);
  if ((rc = dep_axis(H, patch, slide, &ar)) != EBOS_OK || (rc = dep_axis(W, patch, slide, &ac)) != EBOS_OK) return rc;
  EBOS_REQUIRE(row_box && col_box && sel && count, "ebos_gml_dep_select: NULL buffer");
  EBOS_REQUIRE(!thresholding || ((events || n_events == 0) && n_events >= 0 && n_events < ((int64_t)1 << 31) && scratch),
               "ebos_gml_dep_select: bad events or NULL scratch");
  EBOS_REQUIRE(canvas_h >= 0 && canvas_w >= 0 && (int64_t)(canvas_h + 1) * (canvas_w + 1) < ((int64_t)1 << 31),
               "ebos_gml_dep_select: bad canvas %d x %d", canvas_h, canvas_w);
  const hipStream_t st = as_stream(stream);
  const int G = ar.g * ac.g;
  int* sat = static_cast<int*>(scratch);
  const size_t ss = nw > 1 ? scratch_stride / sizeof(int) : 0;
  if (thresholding) {
    const size_t need = (size_t)(canvas_h + 1) * (canvas_w + 1) * sizeof(int);
    if ((rc = gml_check_slices("ebos_gml_dep_select", nw, need, scratch_stride, scratch_bytes)) != EBOS_OK) return rc;
    for (int b = 0; b < nw; ++b)
      if (hipMemsetAsync(static_cast<char*>(scratch) + (size_t)b * scratch_stride, 0, need, st) != hipSuccess) {
        set_error("ebos_gml_dep_select: memset failed");
        return EBOS_ERR_LAUNCH;
      }
    // n_events: one window's count, or the largest count of the batch (it sizes the grid; `offsets` bound each window)
    if (n_events > 0)
      hipLaunchKernelGGL(gml_count_events, dim3(blocks_for(n_events), 1, nw), dim3(kGmlBlock), 0, st, n_events, offsets, events, canvas_h,
                         canvas_w, sat, ss);
    hipLaunchKernelGGL(gml_scan_rows, dim3(blocks_for(canvas_h), 1, nw), dim3(kGmlBlock), 0, st, canvas_h, canvas_w, sat, ss);
    hipLaunchKernelGGL(gml_scan_cols, dim3(blocks_for(canvas_w), 1, nw), dim3(kGmlBlock), 0, st, canvas_h, canvas_w, sat, ss);
  }
  hipLaunchKernelGGL(gml_select, dim3(blocks_for(G), 1, nw), dim3(kGmlBlock), 0, st, ar.g, ac.g, row_box, col_box,
                     thresholding ? sat : nullptr, ss, canvas_h, canvas_w, thresholding, event_thres, sel);
  hipLaunchKernelGGL(gml_rank, dim3(1, 1, nw), dim3(kGmlBlock), 0, st, G, sel, count);
  EBOS_CHECK_LAUNCH("ebos_gml_dep_select");
  return EBOS_OK;
}

// the dependent solver's strides: the crops and the iteration buffers of a window live in its scratch slice
GmlWin dep_win(int nw, const GmlGeom& g, size_t scratch_stride, size_t history_stride, size_t out) {
  GmlWin win = {};
  if (nw > 1) {
    win.grad = win.field = win.scr = scratch_stride / sizeof(double);
    win.x = (size_t)g.nd * g.gh * g.gw;
    win.sel = (size_t)g.gh * g.gw;
    win.hist = history_stride;
    win.out = out;
  }
  return win;
}

int gml_dep_solve(int nw, int H, int W, int patch, int slide, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags,
                  const double* weights, const int* order, int n_terms, const double* gx, const double* gy, size_t grad_stride,
                  const double* q, const double* we, const double* winv, const int* sel, double* x, int iters, double lr, double* history,
                  size_t history_stride, double* flow_out, void* scratch, size_t scratch_stride, size_t scratch_bytes,
                  ebos_stream_t stream) {
  EBOS_REQUIRE(gml_windows_ok(nw), "ebos_gml_dep_solve: %d windows", nw);
  GmlGeom g;
  int rc = make_dep_geom(&g, H, W, patch, slide, n_dim, xmin, xmax, ymin, ymax, flags, weights, order, n_terms);
  if (rc != EBOS_OK) return rc;
  EBOS_REQUIRE(gx && gy && q && winv && sel && x && scratch && (!g.has_we || we), "ebos_gml_dep_solve_f64: NULL buffer");
  EBOS_REQUIRE(iters >= 0, "ebos_gml_dep_solve_f64: iters %d < 0", iters);
  EBOS_REQUIRE(grad_stride == 0 || grad_stride == (size_t)H * W, "ebos_gml_dep_solve: gradient stride is neither 0 nor H W");
  const int G = g.gh * g.gw;
  const DepLayout D = dep_layout(g.H, g.W, G);
  if ((rc = gml_check_slices("ebos_gml_dep_solve_f64", nw, D.total, scratch_stride, scratch_bytes)) != EBOS_OK) return rc;
  const hipStream_t st = as_stream(stream);
  GmlWin src = {};
  if (nw > 1) {
    src.grad = grad_stride;
    src.field = (size_t)H * W;
  }
  const GmlWin win = dep_win(nw, g, scratch_stride, history_stride, 2 * (size_t)H * W);
  GmlBufs B;
  if ((rc = dep_bufs(g, W, xmin, ymin, D, static_cast<char*>(scratch), gx, gy, q, g.has_we ? we : nullptr, winv, x, sel, src, win.scr, nw,
                     st, &B)) != EBOS_OK)
    return rc;
  return gml_adam_loop(g, dep_out_geom(g, H, W, xmin, ymin), B, win, nw, iters, lr, history, flow_out, st);
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

size_t ebos_gml_scratch_bytes_batch(int H, int W, int min_patch, int n_windows) {
  if (n_windows < 1 || n_windows > ebos::kGmlMaxWindows) return 0;
  return (size_t)n_windows * ebos_gml_scratch_bytes(H, W, min_patch);
}

int ebos_gml_prepare_f64(int H, int W, const double* frame, int use_log, const double* pol, int no_polarity, const double* blur_taps,
                         int blur_radius, const double* weight_taps, int weight_radius, const double* inv_taps, int inv_radius,
                         double* gx, double* gy, double* q, double* we, double* winv, void* scratch, size_t scratch_bytes,
                         ebos_stream_t stream) {
  return ebos::gml_prepare(1, H, W, frame, 0, use_log, pol, no_polarity, blur_taps, blur_radius, weight_taps, weight_radius, inv_taps,
                           inv_radius, gx, gy, q, we, winv, scratch, scratch_bytes, stream);
}

int ebos_gml_prepare_batch_f64(int n_windows, int H, int W, const double* frame, int64_t frame_stride, int use_log, const double* pol,
                               int no_polarity, const double* blur_taps, int blur_radius, const double* weight_taps, int weight_radius,
                               const double* inv_taps, int inv_radius, double* gx, double* gy, double* q, double* we, double* winv,
                               void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(frame_stride >= 0, "ebos_gml_prepare_batch_f64: negative frame stride");
  return ebos::gml_prepare(n_windows, H, W, frame, (size_t)frame_stride, use_log, pol, no_polarity, blur_taps, blur_radius, weight_taps,
                           weight_radius, inv_taps, inv_radius, gx, gy, q, we, winv, scratch, scratch_bytes, stream);
}

int ebos_gml_normalize_f64(int64_t n, double* q, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  return ebos::gml_normalize(1, n, q, scratch, scratch_bytes, stream);
}

int ebos_gml_normalize_batch_f64(int n_windows, int64_t n, double* q, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  return ebos::gml_normalize(n_windows, n, q, scratch, scratch_bytes, stream);
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
  const GmlWin win = {};
  if ((rc = gml_forward_backward(g, B, win, 1, parts, st)) != EBOS_OK) return rc;
  AdamArgs a = {};
  hipLaunchKernelGGL(gml_adam, dim3(blocks_for((int64_t)n_dim * G)), dim3(kGmlBlock), 0, st, g, B, win, a, grad);
  EBOS_CHECK_LAUNCH("ebos_gml_objective_f64");
  return EBOS_OK;
}

int ebos_gml_solve_scale_f64(int H, int W, int patch, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags, const double* weights,
                             const int* order, int n_terms, const double* gx, const double* gy, const double* q, const double* we,
                             const double* winv, double* x, int iters, double lr, double* history, double* flow_out, void* scratch,
                             size_t scratch_bytes, ebos_stream_t stream) {
  return ebos::gml_solve_scale(1, H, W, patch, n_dim, xmin, xmax, ymin, ymax, flags, weights, order, n_terms, gx, gy, 0, q, we, winv, x,
                               iters, lr, history, 0, flow_out, scratch, 0, scratch_bytes, stream);
}

int ebos_gml_solve_scale_batch_f64(int n_windows, int H, int W, int patch, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags,
                                   const double* weights, const int* order, int n_terms, const double* gx, const double* gy,
                                   int64_t grad_stride, const double* q, const double* we, const double* winv, double* x, int iters,
                                   double lr, double* history, int64_t history_stride, double* flow_out, void* scratch,
                                   size_t scratch_stride, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(grad_stride >= 0 && history_stride >= 0, "ebos_gml_solve_scale_batch_f64: negative stride");
  EBOS_REQUIRE(!history || n_windows == 1 || history_stride >= 4 * (int64_t)iters, "ebos_gml_solve_scale_batch_f64: history rows overlap");
  return ebos::gml_solve_scale(n_windows, H, W, patch, n_dim, xmin, xmax, ymin, ymax, flags, weights, order, n_terms, gx, gy,
                               (size_t)grad_stride, q, we, winv, x, iters, lr, history, (size_t)history_stride, flow_out, scratch,
                               scratch_stride, scratch_bytes, stream);
}

}  // extern "C"

extern "C" {

size_t ebos_gml_dep_scratch_bytes(int H, int W, int patch, int slide, int xmin, int xmax, int ymin, int ymax, int canvas_h, int canvas_w) {
  using namespace ebos;
  DepAxis ar, ac;
  if (H < 3 || W < 3 || dep_axis(H, patch, slide, &ar) != EBOS_OK || dep_axis(W, patch, slide, &ac) != EBOS_OK) return 0;
  if (!(0 <= xmin && xmin <= xmax && xmax <= H && 0 <= ymin && ymin <= ymax && ymax <= W) || canvas_h < 0 || canvas_w < 0) return 0;
  const size_t prep = 4 * gml_align((size_t)H * W * sizeof(double)) + gml_align(8 * sizeof(double));
  const size_t solve = dep_layout(xmax - xmin, ymax - ymin, ar.g * ac.g).total;
  const size_t sel = gml_align((size_t)(canvas_h + 1) * (canvas_w + 1) * sizeof(int));
  return std::max(std::max(prep, solve), sel);
}

size_t ebos_gml_dep_scratch_bytes_batch(int H, int W, int patch, int slide, int xmin, int xmax, int ymin, int ymax, int canvas_h,
                                        int canvas_w, int n_windows) {
  if (n_windows < 1 || n_windows > ebos::kGmlMaxWindows) return 0;
  return (size_t)n_windows * ebos_gml_dep_scratch_bytes(H, W, patch, slide, xmin, xmax, ymin, ymax, canvas_h, canvas_w);
}

int ebos_gml_dep_select(int H, int W, int patch, int slide, const int* row_box, const int* col_box, const double* events, int64_t n_events,
                        int canvas_h, int canvas_w, int thresholding, double event_thres, int* sel, int* count, void* scratch,
                        size_t scratch_bytes, ebos_stream_t stream) {
  return ebos::gml_dep_select(1, H, W, patch, slide, row_box, col_box, events, n_events, nullptr, canvas_h, canvas_w, thresholding,
                              event_thres, sel, count, scratch, 0, scratch_bytes, stream);
}

int ebos_gml_dep_select_batch(int n_windows, int H, int W, int patch, int slide, const int* row_box, const int* col_box,
                              const double* events, const int64_t* event_offsets, int64_t max_events, int canvas_h, int canvas_w,
                              int thresholding, double event_thres, int* sel, int* count, void* scratch, size_t scratch_stride,
                              size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(!thresholding || event_offsets, "ebos_gml_dep_select_batch: NULL event offsets");
  return ebos::gml_dep_select(n_windows, H, W, patch, slide, row_box, col_box, events, max_events, event_offsets, canvas_h, canvas_w,
                              thresholding, event_thres, sel, count, scratch, scratch_stride, scratch_bytes, stream);
}

int ebos_gml_dep_init_f64(int gh, int gw, int n_dim, const int* sel, const double* draws, double* x, ebos_stream_t stream) {
  return ebos_gml_dep_init_batch_f64(1, gh, gw, n_dim, sel, draws, x, stream);
}

int ebos_gml_dep_init_batch_f64(int n_windows, int gh, int gw, int n_dim, const int* sel, const double* draws, double* x,
                                ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(gml_windows_ok(n_windows) && gh >= 1 && gw >= 1 && n_dim >= 1 && n_dim <= 4 && sel && x,
               "ebos_gml_dep_init_f64: bad arguments");
  const int G = gh * gw;
  hipLaunchKernelGGL(gml_dep_init, dim3(blocks_for(G), 1, n_windows), dim3(kGmlBlock), 0, as_stream(stream), G, n_dim, sel, draws, x);
  EBOS_CHECK_LAUNCH("ebos_gml_dep_init_f64");
  return EBOS_OK;
}

int ebos_gml_dep_objective_f64(int H, int W, int patch, int slide, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags,
                               const double* weights, const int* order, int n_terms, const double* gx, const double* gy, const double* q,
                               const double* we, const double* winv, const int* sel, const double* x, double* parts, double* grad,
                               void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  GmlGeom g;
  int rc = make_dep_geom(&g, H, W, patch, slide, n_dim, xmin, xmax, ymin, ymax, flags, weights, order, n_terms);
  if (rc != EBOS_OK) return rc;
  EBOS_REQUIRE(gx && gy && q && winv && sel && x && parts && grad && scratch && (!g.has_we || we), "ebos_gml_dep_objective_f64: NULL buffer");
  const int G = g.gh * g.gw;
  const DepLayout D = dep_layout(g.H, g.W, G);
  if (scratch_bytes < D.total) {
    set_error("ebos_gml_dep_objective_f64: scratch too small (%zu < %zu)", scratch_bytes, D.total);
    return EBOS_ERR_SCRATCH;
  }
  const hipStream_t st = as_stream(stream);
  const GmlWin win = {};
  GmlBufs B;
  if ((rc = dep_bufs(g, W, xmin, ymin, D, static_cast<char*>(scratch), gx, gy, q, g.has_we ? we : nullptr, winv, const_cast<double*>(x),
                     sel, win, 0, 1, st, &B)) != EBOS_OK)
    return rc;
  if ((rc = gml_forward_backward(g, B, win, 1, parts, st)) != EBOS_OK) return rc;
  AdamArgs a = {};
  hipLaunchKernelGGL(gml_adam, dim3(blocks_for((int64_t)n_dim * G)), dim3(kGmlBlock), 0, st, g, B, win, a, grad);
  EBOS_CHECK_LAUNCH("ebos_gml_dep_objective_f64");
  return EBOS_OK;
}

int ebos_gml_dep_solve_f64(int H, int W, int patch, int slide, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags,
                           const double* weights, const int* order, int n_terms, const double* gx, const double* gy, const double* q,
                           const double* we, const double* winv, const int* sel, double* x, int iters, double lr, double* history,
                           double* flow_out, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  return ebos::gml_dep_solve(1, H, W, patch, slide, n_dim, xmin, xmax, ymin, ymax, flags, weights, order, n_terms, gx, gy, 0, q, we, winv,
                             sel, x, iters, lr, history, 0, flow_out, scratch, 0, scratch_bytes, stream);
}

int ebos_gml_dep_solve_batch_f64(int n_windows, int H, int W, int patch, int slide, int n_dim, int xmin, int xmax, int ymin, int ymax,
                                 int flags, const double* weights, const int* order, int n_terms, const double* gx, const double* gy,
                                 int64_t grad_stride, const double* q, const double* we, const double* winv, const int* sel, double* x,
                                 int iters, double lr, double* history, int64_t history_stride, double* flow_out, void* scratch,
                                 size_t scratch_stride, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(grad_stride >= 0 && history_stride >= 0, "ebos_gml_dep_solve_batch_f64: negative stride");
  EBOS_REQUIRE(!history || n_windows == 1 || history_stride >= 4 * (int64_t)iters, "ebos_gml_dep_solve_batch_f64: history rows overlap");
  return ebos::gml_dep_solve(n_windows, H, W, patch, slide, n_dim, xmin, xmax, ymin, ymax, flags, weights, order, n_terms, gx, gy,
                             (size_t)grad_stride, q, we, winv, sel, x, iters, lr, history, (size_t)history_stride, flow_out, scratch,
                             scratch_stride, scratch_bytes, stream);
}

}  // extern "C"
