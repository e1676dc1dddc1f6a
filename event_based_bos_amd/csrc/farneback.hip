// farneback.hip -- dense optical flow between frame pairs, OpenCV's calcOpticalFlowFarneback (flags 0), for a batch of pairs: the
// frame-based flow the reference scores every event-based estimate against (src/frame_flow_estimator.py:30-95 through
// src/utils/frame_utils.py:160-183, cv2.calcOpticalFlowFarneback with the YAML's params_opencv_flow).
//
// The algorithm and its float32 / float64 split are restated in numpy in tests/_farneback_ref.py; every float32 operation here is the
// same IEEE operation in the same order (fp contraction is off), so the kernels reproduce that restatement up to the float64 window
// sums, whose order differs.  Per level k = levels' .. 0 (levels' cut where a side would fall below 32 pixels):
//   fb_level_image     the level image of every frame: the full-resolution frame (uint8 / float32 / float64, converted as
//                      convertTo(CV_32F)) Gaussian-blurred (s x s, sigma_k, BORDER_REFLECT_101; row pass, then column pass) and resized
//                      INTER_LINEAR to (h_k, w_k).  Only the source points the resize reads are blurred;
//   fb_poly_exp        the (2n+1)-tap polynomial expansion R [5] of every level image (vertical pass float32, horizontal float64);
//   fb_init_matrices   the starting flow (zero at the coarsest level, else the coarser flow resized INTER_LINEAR times 1 / pyr_scale)
//                      and M [5] = UpdateMatrices(R0, R1, flow) per pixel;
//   fb_blur_solve      once per iteration: the (2m+1)^2 replicate-border window sum of M in float64, the regularised 2 x 2 solve,
//                      and -- UpdateMatrices being pointwise in the flow -- the next M from the new flow in the same pass (M is
//                      ping-ponged).  The last pass of level 0 writes the caller's output view.
// All launches go on the caller's stream; there is no host synchronisation and there are no atomics, so a pair's result has the same
// bits alone or in a batch and from run to run.  The batch is the grid's z dimension.
#pragma clang fp contract(off)

#include <math.h>

#include <vector>

#include "common.h"

namespace ebos {
namespace {

constexpr int kFbTx = 16, kFbTy = 16;   // 256-thread workgroups over a 16 x 16 pixel tile
constexpr int kFbMaxHalf = 256;         // Gaussian blur half-width limit (s <= 511)
constexpr int kFbMaxPolyN = 7;
constexpr int kFbMinSize = 32;          // OpenCV's min_size of the level rule

struct FbLevelPlan {
  int h, w, r;                          // level size, blur half-width (s = 2r + 1)
  double scale, sigma;
};

struct FbBlurTaps {
  float k[kFbMaxHalf + 1];              // k[0] centre tap, k[j] the taps at +-j
};

struct FbPolyTaps {
  float g[kFbMaxPolyN + 1], xg[kFbMaxPolyN + 1], xxg[kFbMaxPolyN + 1];   // index k = |x|
  double ig11, ig03, ig33, ig55;
};

int fb_round(double v) { return (int)nearbyint(v); }   // cvRound: half to even

std::vector<FbLevelPlan> fb_plan(int H, int W, double pyr_scale, int levels) {
  double scale = 1;
  int k = 0;
  for (; k < levels; k++) {
    scale *= pyr_scale;
    if (W * scale < kFbMinSize || H * scale < kFbMinSize) break;
  }
  std::vector<FbLevelPlan> plan;
  for (int lv = k; lv >= 0; lv--) {
    double s = 1;
    for (int i = 0; i < lv; i++) s *= pyr_scale;
    FbLevelPlan p;
    p.scale = s;
    p.sigma = (1. / s - 1) * 0.5;
    int ks = fb_round(p.sigma * 5) | 1;
    if (ks < 3) ks = 3;
    p.r = ks / 2;
    p.h = fb_round(H * s);
    p.w = fb_round(W * s);
    plan.push_back(p);
  }
  return plan;
}

// getGaussianKernel(2r + 1, sigma, CV_32F): float taps normalised in double; sigma <= 0 (level 0, s = 3) is the fixed [1/4, 1/2, 1/4]
void fb_blur_taps(int r, double sigma, FbBlurTaps* t) {
  const int n = 2 * r + 1;
  std::vector<float> cf(n);
  if (sigma <= 0) {
    cf = {0.25f, 0.5f, 0.25f};
  } else {
    const double scale2 = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; i++) {
      const double x = i - (n - 1) * 0.5;
      cf[i] = (float)exp(scale2 * x * x);
      sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) cf[i] = (float)(cf[i] * sum);
  }
  for (int j = 0; j <= r; j++) t->k[j] = cf[r + j];
}

// FarnebackPrepareGaussian: taps over x = -n..n and ig11, ig03, ig33, ig55 of the inverse Gram matrix (its {1, x^2, y^2} block
// [[a, b, b], [b, c, d], [b, d, c]] inverted in closed form)
void fb_poly_taps(int n, double sigma, FbPolyTaps* t) {
  if (sigma < 1.1920928955078125e-07) sigma = n * 0.3;
  float g[2 * kFbMaxPolyN + 1], xg[2 * kFbMaxPolyN + 1], xxg[2 * kFbMaxPolyN + 1];
  double s = 0;
  for (int x = -n; x <= n; x++) {
    g[x + n] = (float)exp(-x * x / (2 * sigma * sigma));
    s += g[x + n];
  }
  s = 1. / s;
  for (int x = -n; x <= n; x++) {
    g[x + n] = (float)(g[x + n] * s);
    xg[x + n] = (float)x * g[x + n];
    xxg[x + n] = (float)(x * x) * g[x + n];
  }
  double G00 = 0, G11 = 0, G33 = 0, G55 = 0;
  for (int y = -n; y <= n; y++)
    for (int x = -n; x <= n; x++) {
      const float gg = g[y + n] * g[x + n], fx = (float)x, fy = (float)y;
      G00 += gg;
      G11 += gg * fx * fx;
      G33 += gg * fx * fx * fx * fx;
      G55 += gg * fx * fx * fy * fy;
    }
  const double a = G00, b = G11, c = G33, d = G55;
  const double q = a * (c + d) - 2 * b * b;
  t->ig03 = -b / q;
  t->ig33 = (a * c - b * b) / ((c - d) * q);
  t->ig11 = 1. / G11;
  t->ig55 = 1. / G55;
  for (int k = 0; k <= n; k++) {
    t->g[k] = g[n + k];
    t->xg[k] = xg[n + k];
    t->xxg[k] = xxg[n + k];
  }
}

// ---- device helpers -------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int fb_reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

struct FbLinear {
  int s0, s1;
  float f;   // weight of s1
};

// INTER_LINEAR source taps of destination index d (src -> dst samples): f = (d + 0.5) * (src / dst) - 0.5 in double, rounded to
// float; clamped at both edges with the weight set to 0
__device__ __forceinline__ FbLinear fb_linear(int d, int src, int dst) {
  const double scale = 1. / ((double)dst / src);
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    f = 0.f;
    s = 0;
  }
  if (s >= src - 1) {
    f = 0.f;
    s = src - 1;
  }
  FbLinear l;
  l.s0 = s;
  l.s1 = min(s + 1, src - 1);
  l.f = f;
  return l;
}

template <typename T>
__device__ __forceinline__ float fb_load(const T* p) {
  return (float)*p;
}

// the blurred full-resolution frame at (y, x): the row pass at rows y - r .. y + r, then the column pass
template <typename T>
__device__ float fb_blurred(const T* src, int64_t sr, int H, int W, int y, int x, int r, const FbBlurTaps& t) {
  auto row = [&](int yy) {
    const T* p = src + (int64_t)fb_reflect101(yy, H) * sr;
    float acc = fb_load(p + x) * t.k[0];
    for (int j = 1; j <= r; j++) acc = acc + t.k[j] * (fb_load(p + fb_reflect101(x - j, W)) + fb_load(p + fb_reflect101(x + j, W)));
    return acc;
  };
  float col = row(y) * t.k[0];
  for (int j = 1; j <= r; j++) col = col + t.k[j] * (row(y - j) + row(y + j));
  return col;
}

struct FbImageArgs {
  const void* prev;
  const void* next;
  int64_t prev_sb, prev_sr, next_sb, next_sr;
  int nprev, H, W, h, w, r;
  float* img;   // [nprev + B, h, w]
};

template <typename T>
__global__ void __launch_bounds__(kFbTx* kFbTy) fb_level_image(FbImageArgs a, FbBlurTaps t) {
  const int x = blockIdx.x * kFbTx + threadIdx.x, y = blockIdx.y * kFbTy + threadIdx.y, z = blockIdx.z;
  if (x >= a.w || y >= a.h) return;
  const T* src;
  int64_t sr;
  if (z < a.nprev) {
    src = static_cast<const T*>(a.prev) + z * a.prev_sb;
    sr = a.prev_sr;
  } else {
    src = static_cast<const T*>(a.next) + (int64_t)(z - a.nprev) * a.next_sb;
    sr = a.next_sr;
  }
  float v;
  if (a.h == a.H && a.w == a.W) {
    v = fb_blurred(src, sr, a.H, a.W, y, x, a.r, t);
  } else {
    const FbLinear lx = fb_linear(x, a.W, a.w), ly = fb_linear(y, a.H, a.h);
    const float fx1 = 1.f - lx.f, fy1 = 1.f - ly.f;
    const float t0 = fb_blurred(src, sr, a.H, a.W, ly.s0, lx.s0, a.r, t) * fx1 +
                     fb_blurred(src, sr, a.H, a.W, ly.s0, lx.s1, a.r, t) * lx.f;
    const float t1 = fb_blurred(src, sr, a.H, a.W, ly.s1, lx.s0, a.r, t) * fx1 +
                     fb_blurred(src, sr, a.H, a.W, ly.s1, lx.s1, a.r, t) * lx.f;
    v = t0 * fy1 + t1 * ly.f;
  }
  a.img[((int64_t)z * a.h + y) * a.w + x] = v;
}

// FarnebackPolyExp at (y, x) of img [h, w] -> R[c * plane] for c = 0..4
__global__ void __launch_bounds__(kFbTx* kFbTy) fb_poly_exp(const float* __restrict__ img, float* __restrict__ R, int h, int w, int n,
                                                            FbPolyTaps t) {
  const int x = blockIdx.x * kFbTx + threadIdx.x, y = blockIdx.y * kFbTy + threadIdx.y, z = blockIdx.z;
  if (x >= w || y >= h) return;
  const int64_t plane = (int64_t)h * w;
  const float* src = img + z * plane;
  // vertical pass at column c (replicated rows): v0 = g0 s + sum g_k (up + dn), v1 = sum xg_k (dn - up), v2 = sum xxg_k (up + dn)
  auto vert = [&](int c, float& v0, float& v1, float& v2) {
    v0 = src[(int64_t)y * w + c] * t.g[0];
    v1 = 0.f;
    v2 = 0.f;
    for (int k = 1; k <= n; k++) {
      const float up = src[(int64_t)max(y - k, 0) * w + c], dn = src[(int64_t)min(y + k, h - 1) * w + c];
      const float p = up + dn;
      v0 = v0 + t.g[k] * p;
      v1 = v1 + t.xg[k] * (dn - up);
      v2 = v2 + t.xxg[k] * p;
    }
  };
  float c0, c1, c2;
  vert(x, c0, c1, c2);
  double b1 = (double)(c0 * t.g[0]), b3 = (double)(c1 * t.g[0]), b5 = (double)(c2 * t.g[0]), b2 = 0, b4 = 0, b6 = 0;
  for (int k = 1; k <= n; k++) {
    float l0, l1, l2, r0, r1, r2;
    vert(max(x - k, 0), l0, l1, l2);
    vert(min(x + k, w - 1), r0, r1, r2);
    const double tg = (double)(r0 + l0);
    b1 = b1 + tg * (double)t.g[k];
    b4 = b4 + tg * (double)t.xxg[k];
    b2 = b2 + (double)((r0 - l0) * t.xg[k]);
    b3 = b3 + (double)((r1 + l1) * t.g[k]);
    b6 = b6 + (double)((r1 - l1) * t.xg[k]);
    b5 = b5 + (double)((r2 + l2) * t.g[k]);
  }
  float* out = R + z * 5 * plane + (int64_t)y * w + x;
  out[0] = (float)(b3 * t.ig11);
  out[plane] = (float)(b2 * t.ig11);
  out[2 * plane] = (float)(b1 * t.ig03 + b5 * t.ig33);
  out[3 * plane] = (float)(b1 * t.ig03 + b4 * t.ig33);
  out[4 * plane] = (float)(b6 * t.ig55);
}

__device__ __forceinline__ float fb_border(int d) { return d == 0 || d == 1 ? 0.14f : 0.4472f; }

// FarnebackUpdateMatrices at (y, x) for the flow (dx, dy): R0, R1 [5, h, w] -> M [5] (plane stride `plane`)
__device__ void fb_update_matrices(const float* __restrict__ R0, const float* __restrict__ R1, int h, int w, int y, int x, float dx,
                                   float dy, float* __restrict__ M, int64_t plane) {
  const int64_t o = (int64_t)y * w + x;
  float fx = (float)x + dx, fy = (float)y + dy;
  const int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
  fx -= (float)x1;
  fy -= (float)y1;
  float r2, r3, r4, r5, r6;
  if (x1 >= 0 && x1 < w - 1 && y1 >= 0 && y1 < h - 1) {
    const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
    const int64_t q = (int64_t)y1 * w + x1;
    float r[5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
      const float* p = R1 + c * plane + q;
      r[c] = a00 * p[0] + a01 * p[1] + a10 * p[w] + a11 * p[w + 1];
    }
    r2 = r[0];
    r3 = r[1];
    r4 = (R0[2 * plane + o] + r[2]) * 0.5f;
    r5 = (R0[3 * plane + o] + r[3]) * 0.5f;
    r6 = (R0[4 * plane + o] + r[4]) * 0.25f;
  } else {
    r2 = r3 = 0.f;
    r4 = R0[2 * plane + o];
    r5 = R0[3 * plane + o];
    r6 = R0[4 * plane + o] * 0.5f;
  }
  r2 = (R0[o] - r2) * 0.5f;
  r3 = (R0[plane + o] - r3) * 0.5f;
  r2 = r2 + (r4 * dy + r6 * dx);
  r3 = r3 + (r6 * dy + r5 * dx);
  if (x < 5 || x >= w - 5 || y < 5 || y >= h - 5) {
    const float s = (((x < 5 ? fb_border(x) : 1.f) * (w - 1 - x < 5 ? fb_border(w - 1 - x) : 1.f)) * (y < 5 ? fb_border(y) : 1.f)) *
                    (h - 1 - y < 5 ? fb_border(h - 1 - y) : 1.f);
    r2 *= s;
    r3 *= s;
    r4 *= s;
    r5 *= s;
    r6 *= s;
  }
  M[0] = r4 * r4 + r6 * r6;
  M[plane] = (r4 + r5) * r6;
  M[2 * plane] = r5 * r5 + r6 * r6;
  M[3 * plane] = r4 * r2 + r6 * r3;
  M[4 * plane] = r6 * r2 + r5 * r3;
}

struct FbPairArgs {
  const float* R;        // [nprev + B, 5, h, w]
  int nprev, h, w;
  const float* flow_in;  // fb_init_matrices: the coarser flow [B, 2, hp, wp] (NULL at the coarsest level)
  int hp, wp;
  float inv_scale;       // (float)(1 / pyr_scale)
  float* flow;           // [B, 2, h, w]
  const float* M_in;     // fb_blur_solve: [B, 5, h, w]
  float* M_out;          // [B, 5, h, w]; NULL: the last iteration (no next M)
  int m;                 // window half-width
  double box_scale;      // 1 / winsize^2
  float* out;            // not NULL: write the flow here instead of `flow` (strides below, in elements)
  int64_t out_sb, out_sc, out_sr, out_sx;
};

__device__ __forceinline__ const float* fb_R0(const FbPairArgs& a, int b) {
  return a.R + (int64_t)(a.nprev == 1 ? 0 : b) * 5 * a.h * a.w;
}
__device__ __forceinline__ const float* fb_R1(const FbPairArgs& a, int b) {
  return a.R + (int64_t)(a.nprev + b) * 5 * a.h * a.w;
}

__global__ void __launch_bounds__(kFbTx* kFbTy) fb_init_matrices(FbPairArgs a) {
  const int x = blockIdx.x * kFbTx + threadIdx.x, y = blockIdx.y * kFbTy + threadIdx.y, b = blockIdx.z;
  if (x >= a.w || y >= a.h) return;
  const int64_t plane = (int64_t)a.h * a.w, o = (int64_t)y * a.w + x;
  float dx = 0.f, dy = 0.f;
  if (a.flow_in) {
    const int64_t pp = (int64_t)a.hp * a.wp;
    const float* f = a.flow_in + b * 2 * pp;
    float v[2];
    if (a.hp == a.h && a.wp == a.w) {
      v[0] = f[o];
      v[1] = f[pp + o];
    } else {
      const FbLinear lx = fb_linear(x, a.wp, a.w), ly = fb_linear(y, a.hp, a.h);
      const float fx1 = 1.f - lx.f, fy1 = 1.f - ly.f;
#pragma unroll
      for (int c = 0; c < 2; c++) {
        const float* p = f + c * pp;
        const float t0 = p[(int64_t)ly.s0 * a.wp + lx.s0] * fx1 + p[(int64_t)ly.s0 * a.wp + lx.s1] * lx.f;
        const float t1 = p[(int64_t)ly.s1 * a.wp + lx.s0] * fx1 + p[(int64_t)ly.s1 * a.wp + lx.s1] * lx.f;
        v[c] = t0 * fy1 + t1 * ly.f;
      }
    }
    dx = v[0] * a.inv_scale;
    dy = v[1] * a.inv_scale;
  }
  float* fl = a.flow + b * 2 * plane + o;
  fl[0] = dx;
  fl[plane] = dy;
  fb_update_matrices(fb_R0(a, b), fb_R1(a, b), a.h, a.w, y, x, dx, dy, a.M_out + b * 5 * plane + o, plane);
}

__global__ void __launch_bounds__(kFbTx* kFbTy) fb_blur_solve(FbPairArgs a) {
  const int x = blockIdx.x * kFbTx + threadIdx.x, y = blockIdx.y * kFbTy + threadIdx.y, b = blockIdx.z;
  if (x >= a.w || y >= a.h) return;
  const int64_t plane = (int64_t)a.h * a.w, o = (int64_t)y * a.w + x;
  const float* M = a.M_in + b * 5 * plane;
  double s[5] = {0, 0, 0, 0, 0};
  for (int i = -a.m; i <= a.m; i++) {
    const float* row = M + (int64_t)min(max(y + i, 0), a.h - 1) * a.w;
    for (int j = -a.m; j <= a.m; j++) {
      const int c = min(max(x + j, 0), a.w - 1);
#pragma unroll
      for (int k = 0; k < 5; k++) s[k] += (double)row[k * plane + c];
    }
  }
  const double g11 = s[0] * a.box_scale, g12 = s[1] * a.box_scale, g22 = s[2] * a.box_scale, h1 = s[3] * a.box_scale,
               h2 = s[4] * a.box_scale;
  const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
  const float dx = (float)((g11 * h2 - g12 * h1) * idet), dy = (float)((g22 * h1 - g12 * h2) * idet);
  if (a.out) {
    float* p = a.out + b * a.out_sb + y * a.out_sr + x * a.out_sx;
    p[0] = dx;
    p[a.out_sc] = dy;
  } else {
    float* fl = a.flow + b * 2 * plane + o;
    fl[0] = dx;
    fl[plane] = dy;
  }
  if (a.M_out) fb_update_matrices(fb_R0(a, b), fb_R1(a, b), a.h, a.w, y, x, dx, dy, a.M_out + b * 5 * plane + o, plane);
}

struct FbLayout {
  size_t img, R, flow0, flow1, M0, M1, total;
};

size_t fb_align(size_t b) { return (b + 255) & ~(size_t)255; }

FbLayout fb_layout(int B, int H, int W, int nprev) {
  const size_t hw = (size_t)H * W * sizeof(float), n = (size_t)(nprev + B);
  FbLayout L;
  L.img = 0;
  L.R = fb_align(L.img + n * hw);
  L.flow0 = fb_align(L.R + n * 5 * hw);
  L.flow1 = fb_align(L.flow0 + (size_t)B * 2 * hw);
  L.M0 = fb_align(L.flow1 + (size_t)B * 2 * hw);
  L.M1 = fb_align(L.M0 + (size_t)B * 5 * hw);
  L.total = fb_align(L.M1 + (size_t)B * 5 * hw);
  return L;
}

template <typename T>
int fb_launch_level_image(const FbImageArgs& a, const FbBlurTaps& t, dim3 grid, hipStream_t st) {
  fb_level_image<T><<<grid, dim3(kFbTx, kFbTy), 0, st>>>(a, t);
  EBOS_CHECK_LAUNCH("fb_level_image");
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

size_t ebos_farneback_scratch_bytes(int B, int H, int W, int prev_shared) {
  if (B <= 0 || H < 2 || W < 2) return 0;
  return ebos::fb_layout(B, H, W, prev_shared ? 1 : B).total;
}

int ebos_farneback(int in_dtype, int B, int H, int W, const void* prev, int64_t prev_sb, int64_t prev_sr, const void* next,
                   int64_t next_sb, int64_t next_sr, double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                   double poly_sigma, int flags, float* out, int64_t out_sb, int64_t out_sc, int64_t out_sr, int64_t out_sx,
                   void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(in_dtype == EBOS_FARNEBACK_U8 || in_dtype == EBOS_FARNEBACK_F32 || in_dtype == EBOS_FARNEBACK_F64,
               "ebos_farneback: in_dtype %d is not U8 (0), F32 (1) or F64 (2)", in_dtype);
  EBOS_REQUIRE(B > 0 && B < 65535 && H >= 2 && W >= 2 && (int64_t)H * W < ((int64_t)1 << 31), "ebos_farneback: bad shape B = %d, H = %d, W = %d",
               B, H, W);
  EBOS_REQUIRE(pyr_scale > 0 && pyr_scale < 1 && levels >= 0 && winsize >= 1 && iterations >= 1 && (poly_n == 5 || poly_n == 7),
               "ebos_farneback: bad parameters pyr_scale %g, levels %d, winsize %d, iterations %d, poly_n %d", pyr_scale, levels, winsize,
               iterations, poly_n);
  if (flags != 0) {
    set_error("ebos_farneback: flags %d are not supported (only 0)", flags);
    return EBOS_ERR_UNSUPPORTED;
  }
  EBOS_REQUIRE(prev && next && out && scratch, "ebos_farneback: NULL buffer");
  EBOS_REQUIRE(prev_sb >= 0 && prev_sr >= W && next_sb >= 0 && next_sr >= W && out_sb >= 0 && out_sc >= 0 && out_sr >= 0 && out_sx >= 0,
               "ebos_farneback: bad strides");
  const int nprev = prev_sb == 0 ? 1 : B;
  const size_t need = ebos_farneback_scratch_bytes(B, H, W, nprev == 1);
  if (scratch_bytes < need) {
    set_error("ebos_farneback: scratch too small (%zu < %zu)", scratch_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  EBOS_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 16 == 0, "ebos_farneback: scratch not 16-byte aligned");
  const std::vector<FbLevelPlan> plan = fb_plan(H, W, pyr_scale, levels);
  for (const FbLevelPlan& p : plan)
    EBOS_REQUIRE(p.r <= kFbMaxHalf && p.h >= 1 && p.w >= 1, "ebos_farneback: level %d x %d needs a blur of %d taps (at most %d)", p.h, p.w,
                 2 * p.r + 1, 2 * kFbMaxHalf + 1);
  FbPolyTaps pt;
  fb_poly_taps(poly_n, poly_sigma, &pt);
  const FbLayout L = fb_layout(B, H, W, nprev);
  char* s = static_cast<char*>(scratch);
  float* img = reinterpret_cast<float*>(s + L.img);
  float* R = reinterpret_cast<float*>(s + L.R);
  float* flows[2] = {reinterpret_cast<float*>(s + L.flow0), reinterpret_cast<float*>(s + L.flow1)};
  float* Ms[2] = {reinterpret_cast<float*>(s + L.M0), reinterpret_cast<float*>(s + L.M1)};
  const hipStream_t st = as_stream(stream);
  const float* coarser = nullptr;
  int hp = 0, wp = 0, cur = 0;
  for (size_t li = 0; li < plan.size(); li++) {
    const FbLevelPlan& p = plan[li];
    const bool finest = li + 1 == plan.size();
    const dim3 tiles((p.w + kFbTx - 1) / kFbTx, (p.h + kFbTy - 1) / kFbTy);
    FbBlurTaps bt;
    fb_blur_taps(p.r, p.sigma, &bt);   // (sigma 0 at level 0: the fixed 3-tap kernel)
    FbImageArgs ia = {prev, next, prev_sb, prev_sr, next_sb, next_sr, nprev, H, W, p.h, p.w, p.r, img};
    const dim3 gi(tiles.x, tiles.y, nprev + B);
    int rc = in_dtype == EBOS_FARNEBACK_U8    ? fb_launch_level_image<uint8_t>(ia, bt, gi, st)
             : in_dtype == EBOS_FARNEBACK_F32 ? fb_launch_level_image<float>(ia, bt, gi, st)
                                              : fb_launch_level_image<double>(ia, bt, gi, st);
    if (rc != EBOS_OK) return rc;
    fb_poly_exp<<<gi, dim3(kFbTx, kFbTy), 0, st>>>(img, R, p.h, p.w, poly_n, pt);
    EBOS_CHECK_LAUNCH("fb_poly_exp");
    FbPairArgs a = {};
    a.R = R;
    a.nprev = nprev;
    a.h = p.h;
    a.w = p.w;
    a.flow_in = coarser;
    a.hp = hp;
    a.wp = wp;
    a.inv_scale = (float)(1. / pyr_scale);
    a.flow = flows[cur];
    a.m = winsize / 2;
    a.box_scale = 1. / (winsize * winsize);
    a.M_out = Ms[0];
    const dim3 gp(tiles.x, tiles.y, B);
    fb_init_matrices<<<gp, dim3(kFbTx, kFbTy), 0, st>>>(a);
    EBOS_CHECK_LAUNCH("fb_init_matrices");
    a.flow_in = nullptr;
    for (int it = 0; it < iterations; it++) {
      const bool last = it == iterations - 1;
      a.M_in = Ms[it & 1];
      a.M_out = last ? nullptr : Ms[(it + 1) & 1];
      if (last && finest) {
        a.out = out;
        a.out_sb = out_sb;
        a.out_sc = out_sc;
        a.out_sr = out_sr;
        a.out_sx = out_sx;
      }
      fb_blur_solve<<<gp, dim3(kFbTx, kFbTy), 0, st>>>(a);
      EBOS_CHECK_LAUNCH("fb_blur_solve");
    }
    coarser = flows[cur];
    hp = p.h;
    wp = p.w;
    cur ^= 1;
  }
  return EBOS_OK;
}

}  // extern "C"
