// photometric.hip -- does a flow explain the two camera frames it was estimated between?
//   ebos_warp_image_forward_{f32,f64}  the reference's warp_image_forward / warp_image_torch (src/utils/frame_utils.py:56-115): the image
//                                      sampled at x - flow, bilinear, zeros outside (the chain of image_warp.h)
//   ebos_ssim_map_{f32,f64}            the reference's SSIM map (src/utils/stat_utils.py:215-285): five windowed moments E[x], E[y], E[x x],
//                                      E[y y], E[x y] under the host's 2-D taps, zero padding of window_size / 2, then
//                                      ((2 mx my + C1)(2 sxy + C2)) / ((mx mx + my my + C1)(sxx + syy + C2)); optionally its means
//   ebos_photometric_batch             per item L1, RMSE and mean SSIM of (warp(frame1, flow), frame2) and of (frame1, frame2) over the
//                                      counted pixels, and their count
// Every product and sum is rounded on its own (the file is compiled with -ffp-contract=off): the results differ from the
// reference's by the order of the window sums alone.
//
// The SSIM tile: one workgroup of 256 threads per 16-row tile per item, a thread owns the 16 bytes of a row that one ds_read_b128
// covers (4 float32 / 2 float64 pixels), a wave covers 4 rows x 16 threads.  Both images' tile plus halo live in LDS in rows of
// 512 bytes: ds_read_b128 is served in groups of 16 lanes that span two of the wave's rows ({0-3, 12-15, 20-27}, ...), and with a
// row stride that is a multiple of 256 bytes the 16 lanes of a group fall on 16 different 16-byte bank quadruples whatever rows
// they sit in -- the inner reads are conflict-free.  Per window row a thread reads the 16 (14) elements its pixels need from each
// image once, forms the three products, and walks the row's taps, which are read through the scalar unit (a wave-uniform index).
// The default window of 11 has kernels of its own (WS = 11: the tap loop is fully unrolled and every LDS read is a ds_read_b128); the
// other odd sizes up to 13 share one (WS = 0: the unrolled tap loop skips the taps beyond the window with a wave-uniform branch).
//
// The fused score fills three such tiles -- warp(frame1), frame2, frame1 -- plus a byte per pixel "all four taps inside and the flow
// finite", evaluates the SSIM strip twice with the function ebos_ssim_map uses (the same bits), and reduces |d|, d d and both SSIM
// values over the counted pixels in float64 pairs (hi + lo, error-free additions: the sum does not depend on its order): thread,
// wave, workgroup -> one record per tile; a second launch sums an item's records.  No atomics, no host synchronisation, the same
// bits on every run and at every place in a batch.
#include "common.h"
#include "image_warp.h"

namespace ebos {
namespace {

constexpr int kPhBlock = 256;
constexpr int kPhWaves = kPhBlock / kWave;
constexpr int kPhTileH = 16;
constexpr int kPhWindow = 11;      // the reference's default window: kernels with the window size fixed at compile time
constexpr int kPhMaxWindow = 13;   // the largest window of the kernels that take the size at run time
constexpr int kPhMaxPad = kPhMaxWindow / 2;
constexpr int kPhRows = kPhTileH + 2 * kPhMaxPad;   // 28 LDS rows
constexpr int kPhRowBytes = 512;
constexpr int kPhSums = 6;                          // L1, squared error, SSIM; the same for the un-warped frame

template <typename T>
struct PhGeom {
  static constexpr int PX = 16 / (int)sizeof(T);           // pixels per thread: one 16-byte LDS read
  static constexpr int TW = 16 * PX;                        // tile width: 64 (float32) / 32 (float64)
  static constexpr int STRIDE = kPhRowBytes / (int)sizeof(T);
  static constexpr int NV = (kPhMaxWindow - 1 + PX + PX - 1) / PX;   // 16-byte reads per window row: 4 / 7
  static constexpr int NE = NV * PX;                        // elements a thread holds per window row: 16 / 14
  static constexpr int LW = TW + 2 * kPhMaxPad;             // columns of an LDS row that are filled: 76 / 44 (>= 15 PX + NE)
};

template <typename T>
struct alignas(16) PhVec {
  T v[16 / sizeof(T)];
};

// SSIM at the PX pixels of thread (ty, tx) from the two tiles in LDS (row 0 = the tile's first row minus pad).
template <typename T, int WS>
__device__ __forceinline__ void ssim_strip(const T* __restrict__ sa, const T* __restrict__ sb, const T* __restrict__ taps, int ws_rt,
                                           int ty, int tx, T c1, T c2, T* __restrict__ out) {
  using G = PhGeom<T>;
  const int ws = WS ? WS : ws_rt;
  T m1[G::PX], m2[G::PX], e11[G::PX], e22[G::PX], e12[G::PX];
#pragma unroll
  for (int j = 0; j < G::PX; ++j) m1[j] = m2[j] = e11[j] = e22[j] = e12[j] = T(0);
  for (int dy = 0; dy < ws; ++dy) {
    const T* ra = sa + (ty + dy) * G::STRIDE + G::PX * tx;
    const T* rb = sb + (ty + dy) * G::STRIDE + G::PX * tx;
    T a[G::NE], b[G::NE], aa[G::NE], bb[G::NE], ab[G::NE];
#pragma unroll
    for (int k = 0; k < G::NV; ++k) {
      const PhVec<T> va = *reinterpret_cast<const PhVec<T>*>(ra + k * G::PX);
      const PhVec<T> vb = *reinterpret_cast<const PhVec<T>*>(rb + k * G::PX);
#pragma unroll
      for (int j = 0; j < G::PX; ++j) {
        a[k * G::PX + j] = va.v[j];
        b[k * G::PX + j] = vb.v[j];
      }
    }
#pragma unroll
    for (int k = 0; k < G::NE; ++k) {
      aa[k] = a[k] * a[k];
      bb[k] = b[k] * b[k];
      ab[k] = a[k] * b[k];
    }
    const T* tw = taps + dy * ws;
#pragma unroll
    for (int dx = 0; dx < (WS ? WS : kPhMaxWindow); ++dx) {
      if (WS || dx < ws) {   // (wave-uniform)
        const T w = tw[dx];
#pragma unroll
        for (int j = 0; j < G::PX; ++j) {
          m1[j] += w * a[dx + j];
          m2[j] += w * b[dx + j];
          e11[j] += w * aa[dx + j];
          e22[j] += w * bb[dx + j];
          e12[j] += w * ab[dx + j];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < G::PX; ++j) {
    const T mu1_sq = m1[j] * m1[j], mu2_sq = m2[j] * m2[j], mu12 = m1[j] * m2[j];
    const T s1 = e11[j] - mu1_sq, s2 = e22[j] - mu2_sq, s12 = e12[j] - mu12;
    out[j] = ((T(2) * mu12 + c1) * (T(2) * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2));
  }
}

// ---- float64 sums that do not depend on their order: a sum is carried as an unevaluated pair hi + lo (error-free additions: the
// rounding error of every hi + x goes to lo), so that hi + lo is the exact sum rounded once, for any order of the addends short of a
// near-tie at 2^-100 of the sum.  The means below are therefore the correctly rounded means of the per-pixel values.
struct PhDD {
  double hi, lo;
};
__device__ __forceinline__ void dd_add(PhDD& a, double x) {
  const double s = a.hi + x, bb = s - a.hi;
  a.lo += (a.hi - (s - bb)) + (x - bb);
  a.hi = s;
}
__device__ __forceinline__ PhDD dd_merge(const PhDD& a, const PhDD& b) {
  const double s = a.hi + b.hi, bb = s - a.hi;
  const double e = ((a.hi - (s - bb)) + (b.hi - bb)) + (a.lo + b.lo);
  PhDD r;
  r.hi = s + e;
  r.lo = e - (r.hi - s);
  return r;
}
__device__ __forceinline__ double dd_value(const PhDD& a) { return a.hi + a.lo; }
__device__ __forceinline__ PhDD dd_wave_sum(PhDD v) {   // valid in lane 0
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    PhDD o;
    o.hi = __shfl_down(v.hi, off, kWave);
    o.lo = __shfl_down(v.lo, off, kWave);
    v = dd_merge(v, o);
  }
  return v;
}
// workgroup-wide: wave, then the waves in index order; valid in thread 0
__device__ __forceinline__ PhDD dd_block_sum(PhDD v, PhDD* s_red) {
  v = dd_wave_sum(v);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  __syncthreads();   // (s_red is reused from one call to the next)
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  PhDD t = s_red[0];
  for (int w = 1; w < kPhWaves; ++w) t = dd_merge(t, s_red[w]);
  return t;
}

struct PhTile {
  int r0, c0;   // the tile's first pixel
};
template <typename T>
__device__ __forceinline__ PhTile ph_tile(int tiles_x) {
  PhTile t;
  t.r0 = ((int)blockIdx.x / tiles_x) * kPhTileH;
  t.c0 = ((int)blockIdx.x % tiles_x) * PhGeom<T>::TW;
  return t;
}

template <typename T, int WS>
__global__ __launch_bounds__(kPhBlock) void ssim_map_kernel(const T* __restrict__ img1, const T* __restrict__ img2,
                                                            const T* __restrict__ taps, int ws_rt, int H, int W, int tiles_x, T c1, T c2,
                                                            T* __restrict__ out, PhDD* __restrict__ part) {
  const int ws = WS ? WS : ws_rt;
  using G = PhGeom<T>;
  __shared__ PhVec<T> sa_v[kPhRows * kPhRowBytes / 16], sb_v[kPhRows * kPhRowBytes / 16];
  T* sa = reinterpret_cast<T*>(sa_v);
  T* sb = reinterpret_cast<T*>(sb_v);
  const PhTile t = ph_tile<T>(tiles_x);
  const int pad = ws / 2, rows = kPhTileH + 2 * pad;
  const size_t base = (size_t)blockIdx.y * H * W;
  for (int i = threadIdx.x; i < rows * G::LW; i += kPhBlock) {
    const int lr = i / G::LW, lc = i % G::LW;
    const int r = t.r0 - pad + lr, c = t.c0 - pad + lc;
    const bool in = r >= 0 && r < H && c >= 0 && c < W;
    sa[lr * G::STRIDE + lc] = in ? img1[base + (size_t)r * W + c] : T(0);
    sb[lr * G::STRIDE + lc] = in ? img2[base + (size_t)r * W + c] : T(0);
  }
  __syncthreads();
  const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
  T v[G::PX];
  ssim_strip<T, WS>(sa, sb, taps, ws, ty, tx, c1, c2, v);
  const int r = t.r0 + ty;
#pragma unroll
  for (int j = 0; j < G::PX; ++j) {
    const int c = t.c0 + G::PX * tx + j;
    if (r < H && c < W) out[base + (size_t)r * W + c] = v[j];
  }
  if (part) {   // the tile's sum of the map, for the means (wave-uniform)
    __shared__ PhDD s_red[kPhWaves];
    PhDD s = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < G::PX; ++j)
      if (r < H && t.c0 + G::PX * tx + j < W) dd_add(s, (double)v[j]);
    s = dd_block_sum(s, s_red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

// means[n] = the mean of map n, n < N; sums[n] = its sum: one workgroup per map merges the map's per-tile sums
__global__ __launch_bounds__(kPhBlock) void ssim_map_means(const PhDD* __restrict__ part, int tiles, int64_t HW, double* __restrict__ means,
                                                           PhDD* __restrict__ sums) {
  __shared__ PhDD s_red[kPhWaves];
  const PhDD* p = part + (size_t)blockIdx.x * tiles;
  PhDD s = {0.0, 0.0};
  for (int k = threadIdx.x; k < tiles; k += kPhBlock) s = dd_merge(s, p[k]);
  s = dd_block_sum(s, s_red);
  if (threadIdx.x == 0) {
    means[blockIdx.x] = dd_value(s) / (double)HW;
    sums[blockIdx.x] = s;
  }
}

// means[N + b] = the mean over item b's C maps, means[N + B] = the mean over all N = B C maps
__global__ __launch_bounds__(kPhBlock) void ssim_means_finish(int B, int C, int64_t HW, double* __restrict__ means,
                                                              const PhDD* __restrict__ sums) {
  const int N = B * C;
  for (int b = threadIdx.x; b < B; b += kPhBlock) {
    PhDD s = sums[b * C];
    for (int c = 1; c < C; ++c) s = dd_merge(s, sums[b * C + c]);
    means[N + b] = dd_value(s) / ((double)C * (double)HW);
  }
  if (threadIdx.x == 0) {
    PhDD s = sums[0];
    for (int n = 1; n < N; ++n) s = dd_merge(s, sums[n]);
    means[N + B] = dd_value(s) / ((double)N * (double)HW);
  }
}

// ---- the warp alone ------------------------------------------------------------------------------------------------------------
// shifts: [B, 2] of float32 (shift_f32) or of T.  warp_image_torch subtracts a 0-dim tensor from the float32 grid, which does not promote
// it: the quotient shift / ((size - 1) / 2) is formed in the shift's type, rounded to float32 and subtracted in float32
template <typename T, typename IT>
__global__ __launch_bounds__(kPhBlock) void warp_image_kernel(const IT* __restrict__ images, int64_t image_sb, const T* __restrict__ flows,
                                                              const void* __restrict__ shifts, int shift_f32, int H, int W,
                                                              T* __restrict__ out) {
  const int b = blockIdx.y;
  const int64_t HW = (int64_t)H * W;
  const IT* img = images + (size_t)b * image_sb;
  for (int64_t i = (int64_t)blockIdx.x * kPhBlock + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kPhBlock) {
    const int r = (int)(i / W), c = (int)(i % W);
    T wy, wx;
    if (flows) {
      wy = warp_normalised<T>(r, H, flows[(size_t)b * 2 * HW + i]);
      wx = warp_normalised<T>(c, W, flows[(size_t)b * 2 * HW + HW + i]);
    } else if (shift_f32) {
      const float* s = static_cast<const float*>(shifts) + 2 * b;
      wy = (T)warp_normalised<float>(r, H, s[0]);
      wx = (T)warp_normalised<float>(c, W, s[1]);
    } else {
      const T* s = static_cast<const T*>(shifts) + 2 * b;
      wy = (T)warp_normalised_f32(r, H, (float)(s[0] / (T)((H - 1) / 2.0)));
      wx = (T)warp_normalised_f32(c, W, (float)(s[1] / (T)((W - 1) / 2.0)));
    }
    const WarpTaps<T> t = warp_taps<T>(warp_unnormalise<T>(wy, H), warp_unnormalise<T>(wx, W), H, W);
    out[(size_t)b * HW + i] = warp_gather<T, IT>(img, H, W, t);
  }
}

// ---- the fused score -----------------------------------------------------------------------------------------------------------
struct PhPartial {
  PhDD s[kPhSums];
  unsigned long long n;
};

struct PhArgs {
  const void* frame1;
  const void* frame2;
  const void* flow;
  const void* taps;
  const uint8_t* mask;   // nullable, [B, H, W] with batch stride mask_sb
  int64_t frame1_sb, mask_sb;
  int ws, H, W, tiles_x, tiles;
  int xmin, xmax, ymin, ymax;   // the counted rectangle (the whole image without a roi)
};

template <typename T, typename IT, int WS>
__global__ __launch_bounds__(kPhBlock) void photometric_tiles(PhArgs a, T c1, T c2, PhPartial* __restrict__ part) {
  using G = PhGeom<T>;
  constexpr int kFlagStride = 80;   // >= LW
  __shared__ PhVec<T> sw_v[kPhRows * kPhRowBytes / 16], s2_v[kPhRows * kPhRowBytes / 16], s1_v[kPhRows * kPhRowBytes / 16];
  __shared__ uint8_t s_ok[kPhRows * kFlagStride];
  __shared__ PhDD s_sum[kPhWaves][kPhSums];
  __shared__ unsigned s_cnt[kPhWaves];
  T* sw = reinterpret_cast<T*>(sw_v);
  T* s2 = reinterpret_cast<T*>(s2_v);
  T* s1 = reinterpret_cast<T*>(s1_v);
  const int H = a.H, W = a.W, ws = WS ? WS : a.ws;
  const PhTile t = ph_tile<T>(a.tiles_x);
  const int pad = ws / 2, rows = kPhTileH + 2 * pad;
  const int b = blockIdx.y;
  const size_t HW = (size_t)H * W;
  const IT* f1 = static_cast<const IT*>(a.frame1) + (size_t)b * a.frame1_sb;
  const IT* f2 = static_cast<const IT*>(a.frame2) + (size_t)b * HW;
  const T* flow = static_cast<const T*>(a.flow) + (size_t)b * 2 * HW;

  for (int i = threadIdx.x; i < rows * G::LW; i += kPhBlock) {
    const int lr = i / G::LW, lc = i % G::LW;
    const int r = t.r0 - pad + lr, c = t.c0 - pad + lc;
    T vw = T(0), v2 = T(0), v1 = T(0);
    bool ok = false;
    if (r >= 0 && r < H && c >= 0 && c < W && lc < G::TW + 2 * pad) {
      const size_t k = (size_t)r * W + c;
      const T u0 = flow[k], u1 = flow[HW + k];
      const WarpTaps<T> tp = warp_taps<T>(warp_unnormalise<T>(warp_normalised<T>(r, H, u0), H),
                                          warp_unnormalise<T>(warp_normalised<T>(c, W, u1), W), H, W);
      vw = warp_gather<T, IT>(f1, H, W, tp);
      v2 = (T)f2[k];
      v1 = (T)f1[k];
      ok = tp.inside && __builtin_isfinite(u0) && __builtin_isfinite(u1);
    }
    sw[lr * G::STRIDE + lc] = vw;
    s2[lr * G::STRIDE + lc] = v2;
    s1[lr * G::STRIDE + lc] = v1;
    s_ok[lr * kFlagStride + lc] = ok ? 1 : 0;
  }
  __syncthreads();

  const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
  const T* taps = static_cast<const T*>(a.taps);
  T q[G::PX], q0[G::PX];
  ssim_strip<T, WS>(sw, s2, taps, ws, ty, tx, c1, c2, q);
  ssim_strip<T, WS>(s1, s2, taps, ws, ty, tx, c1, c2, q0);

  PhDD acc[kPhSums];
#pragma unroll
  for (int k = 0; k < kPhSums; ++k) acc[k].hi = acc[k].lo = 0.0;
  unsigned n = 0;
  const int r = t.r0 + ty;
#pragma unroll
  for (int j = 0; j < G::PX; ++j) {
    const int c = t.c0 + G::PX * tx + j;
    const int lr = ty + pad, lc = G::PX * tx + j + pad;
    bool counted = r < H && c < W && r >= a.xmin && r < a.xmax && c >= a.ymin && c < a.ymax && s_ok[lr * kFlagStride + lc] != 0;
    if (counted && a.mask) counted = a.mask[(size_t)b * a.mask_sb + (size_t)r * W + c] != 0;
    if (counted) {
      const T vw = sw[lr * G::STRIDE + lc], v2 = s2[lr * G::STRIDE + lc], v1 = s1[lr * G::STRIDE + lc];
      const T d = vw - v2, d0 = v1 - v2;
      dd_add(acc[0], (double)__builtin_fabs(d));
      dd_add(acc[1], (double)(d * d));
      dd_add(acc[2], (double)q[j]);
      dd_add(acc[3], (double)__builtin_fabs(d0));
      dd_add(acc[4], (double)(d0 * d0));
      dd_add(acc[5], (double)q0[j]);
      n += 1;
    }
  }
#pragma unroll
  for (int k = 0; k < kPhSums; ++k) acc[k] = dd_wave_sum(acc[k]);
  n = wave_sum(n);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kPhSums; ++k) s_sum[wave][k] = acc[k];
    s_cnt[wave] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    PhPartial p;
#pragma unroll
    for (int k = 0; k < kPhSums; ++k) {
      PhDD s = s_sum[0][k];
      for (int w = 1; w < kPhWaves; ++w) s = dd_merge(s, s_sum[w][k]);
      p.s[k] = s;
    }
    unsigned long long cnt = 0;
    for (int w = 0; w < kPhWaves; ++w) cnt += s_cnt[w];
    p.n = cnt;
    part[(size_t)b * a.tiles + blockIdx.x] = p;
  }
}

// out [B, 7]: L1, RMSE, SSIM, L1_0, RMSE_0, SSIM_0, n_points -- one workgroup per item, thread t sums the records t, t + 256, ...
__global__ __launch_bounds__(kPhBlock) void photometric_finish(const PhPartial* __restrict__ part, int tiles, double* __restrict__ out) {
  __shared__ PhDD s_red[kPhWaves];
  const int b = blockIdx.x;
  const PhPartial* p = part + (size_t)b * tiles;
  PhDD acc[kPhSums + 1];
#pragma unroll
  for (int j = 0; j <= kPhSums; ++j) acc[j].hi = acc[j].lo = 0.0;
  for (int k = threadIdx.x; k < tiles; k += kPhBlock) {
#pragma unroll
    for (int j = 0; j < kPhSums; ++j) acc[j] = dd_merge(acc[j], p[k].s[j]);
    acc[kPhSums].hi += (double)p[k].n;   // (exact: at most 2^31 pixels)
  }
  double s[kPhSums];
#pragma unroll
  for (int j = 0; j < kPhSums; ++j) s[j] = dd_value(dd_block_sum(acc[j], s_red));
  const double cnt = dd_value(dd_block_sum(acc[kPhSums], s_red));
  if (threadIdx.x == 0) {
    double* o = out + (size_t)b * 7;
    const double nan = __builtin_nan("");
    const bool any = cnt > 0.0;
    o[0] = any ? s[0] / cnt : nan;
    o[1] = any ? __builtin_sqrt(s[1] / cnt) : nan;
    o[2] = any ? s[2] / cnt : nan;
    o[3] = any ? s[3] / cnt : nan;
    o[4] = any ? __builtin_sqrt(s[4] / cnt) : nan;
    o[5] = any ? s[5] / cnt : nan;
    o[6] = cnt;
  }
}

template <typename T>
int ph_tiles_x(int W) {
  return (W + PhGeom<T>::TW - 1) / PhGeom<T>::TW;
}
int ph_tiles_y(int H) { return (H + kPhTileH - 1) / kPhTileH; }

bool ph_shape_ok(int N, int H, int W) { return N > 0 && N <= 65535 && H >= 2 && W >= 2 && (int64_t)H * W < ((int64_t)1 << 31); }
bool ph_window_ok(int ws) { return ws >= 1 && (ws & 1) == 1; }

constexpr double kC1 = 0.01 * 0.01, kC2 = 0.03 * 0.03;

template <typename T>
int ssim_map_launch(const char* who, const T* img1, const T* img2, const T* taps, int ws, int B, int C, int H, int W, T* out,
                    double* means, hipStream_t s) {
  const int64_t n64 = (int64_t)B * C;
  EBOS_REQUIRE(B > 0 && C > 0 && n64 <= 65535, "%s: bad batch B = %d, C = %d (1 <= B C <= 65535)", who, B, C);
  EBOS_REQUIRE(ph_shape_ok((int)n64, H, W), "%s: bad shape H = %d, W = %d (both >= 2, H W < 2^31)", who, H, W);
  EBOS_REQUIRE(ph_window_ok(ws), "%s: window_size %d is not a positive odd number", who, ws);
  EBOS_REQUIRE(img1 && img2 && taps && out, "%s: NULL buffer", who);
  if (ws > kPhMaxWindow) {
    set_error("%s: window_size %d > %d is not built", who, ws, kPhMaxWindow);
    return EBOS_ERR_UNSUPPORTED;
  }
  const int N = (int)n64, tx = ph_tiles_x<T>(W);
  const int tiles = tx * ph_tiles_y(H);
  const dim3 grid(tiles, N);
  PhDD* sums = means ? reinterpret_cast<PhDD*>(means + N + B + 1) : nullptr;   // [N], then the tiles' sums [N, tiles]
  PhDD* part = means ? sums + N : nullptr;
  const T c1 = (T)kC1, c2 = (T)kC2;
  if (ws == kPhWindow)
    hipLaunchKernelGGL((ssim_map_kernel<T, kPhWindow>), grid, dim3(kPhBlock), 0, s, img1, img2, taps, ws, H, W, tx, c1, c2, out, part);
  else
    hipLaunchKernelGGL((ssim_map_kernel<T, 0>), grid, dim3(kPhBlock), 0, s, img1, img2, taps, ws, H, W, tx, c1, c2, out, part);
  EBOS_CHECK_LAUNCH("ebos_ssim_map: ssim_map_kernel");
  if (means) {
    hipLaunchKernelGGL(ssim_map_means, dim3(N), dim3(kPhBlock), 0, s, part, tiles, (int64_t)H * W, means, sums);
    EBOS_CHECK_LAUNCH("ebos_ssim_map: ssim_map_means");
    hipLaunchKernelGGL(ssim_means_finish, dim3(1), dim3(kPhBlock), 0, s, B, C, (int64_t)H * W, means, sums);
    EBOS_CHECK_LAUNCH("ebos_ssim_map: ssim_means_finish");
  }
  return EBOS_OK;
}

template <typename T>
int warp_image_launch(const char* who, const void* images, int image_dtype, int64_t image_sb, const T* flows, const void* shifts,
                      int shift_dtype, int B, int H, int W, T* out, hipStream_t s) {
  constexpr int own = sizeof(T) == 8 ? EBOS_IMAGE_F64 : EBOS_IMAGE_F32;
  EBOS_REQUIRE(ph_shape_ok(B, H, W), "%s: bad shape B = %d, H = %d, W = %d (1 <= B <= 65535, H, W >= 2, H W < 2^31)", who, B, H, W);
  EBOS_REQUIRE(images && out, "%s: NULL buffer", who);
  EBOS_REQUIRE((flows != nullptr) != (shifts != nullptr), "%s: exactly one of flows / shifts must be given", who);
  EBOS_REQUIRE(image_sb == 0 || image_sb >= (int64_t)H * W, "%s: image_sb %lld is neither 0 nor >= H W", who, (long long)image_sb);
  EBOS_REQUIRE(image_dtype == EBOS_IMAGE_U8 || image_dtype == own,
               "%s: image dtype code %d is not built (%d = uint8, %d = the compute type)", who, image_dtype, EBOS_IMAGE_U8, own);
  EBOS_REQUIRE(!shifts || shift_dtype == own || shift_dtype == EBOS_IMAGE_F32,
               "%s: shift dtype code %d is not built (%d = float32, %d = the compute type)", who, shift_dtype, EBOS_IMAGE_F32, own);
  const dim3 grid(stream_grid((int64_t)H * W, kPhBlock), B);
  const int sf32 = shifts && shift_dtype == EBOS_IMAGE_F32 && own != EBOS_IMAGE_F32;
  if (image_dtype == EBOS_IMAGE_U8)
    hipLaunchKernelGGL((warp_image_kernel<T, uint8_t>), grid, dim3(kPhBlock), 0, s, static_cast<const uint8_t*>(images), image_sb, flows,
                       shifts, sf32, H, W, out);
  else
    hipLaunchKernelGGL((warp_image_kernel<T, T>), grid, dim3(kPhBlock), 0, s, static_cast<const T*>(images), image_sb, flows, shifts, sf32,
                       H, W, out);
  EBOS_CHECK_LAUNCH("ebos_warp_image_forward: warp_image_kernel");
  return EBOS_OK;
}

template <typename T, typename IT>
void photometric_tiles_launch(const PhArgs& a, int B, PhPartial* part, hipStream_t s) {
  const dim3 grid(a.tiles, B);
  if (a.ws == kPhWindow) hipLaunchKernelGGL((photometric_tiles<T, IT, kPhWindow>), grid, dim3(kPhBlock), 0, s, a, (T)kC1, (T)kC2, part);
  else hipLaunchKernelGGL((photometric_tiles<T, IT, 0>), grid, dim3(kPhBlock), 0, s, a, (T)kC1, (T)kC2, part);
}

template <typename T>
int photometric_launch(const PhArgs& a, int frame_dtype, int B, PhPartial* part, double* out, hipStream_t s) {
  if (frame_dtype == EBOS_IMAGE_U8) photometric_tiles_launch<T, uint8_t>(a, B, part, s);
  else photometric_tiles_launch<T, T>(a, B, part, s);
  EBOS_CHECK_LAUNCH("ebos_photometric_batch: photometric_tiles");
  hipLaunchKernelGGL(photometric_finish, dim3(B), dim3(kPhBlock), 0, s, part, a.tiles, out);
  EBOS_CHECK_LAUNCH("ebos_photometric_batch: photometric_finish");
  return EBOS_OK;
}

int ph_tiles(int dtype, int H, int W) {
  return (dtype == EBOS_IMAGE_F64 ? ph_tiles_x<double>(W) : ph_tiles_x<float>(W)) * ph_tiles_y(H);
}

}  // namespace
}  // namespace ebos

extern "C" {

int ebos_warp_image_forward_f32(const void* images, int image_dtype, int64_t image_sb, const float* flows, const void* shifts,
                                int shift_dtype, int B, int H, int W, float* out, ebos_stream_t stream) {
  return ebos::warp_image_launch<float>("ebos_warp_image_forward_f32", images, image_dtype, image_sb, flows, shifts, shift_dtype, B, H, W, out,
                                        ebos::as_stream(stream));
}

int ebos_warp_image_forward_f64(const void* images, int image_dtype, int64_t image_sb, const double* flows, const void* shifts,
                                int shift_dtype, int B, int H, int W, double* out, ebos_stream_t stream) {
  return ebos::warp_image_launch<double>("ebos_warp_image_forward_f64", images, image_dtype, image_sb, flows, shifts, shift_dtype, B, H, W, out,
                                         ebos::as_stream(stream));
}

int ebos_ssim_map_f32(const float* img1, const float* img2, const float* taps, int window_size, int B, int C, int H, int W, float* out,
                      double* means, ebos_stream_t stream) {
  return ebos::ssim_map_launch<float>("ebos_ssim_map_f32", img1, img2, taps, window_size, B, C, H, W, out, means, ebos::as_stream(stream));
}

int ebos_ssim_map_f64(const double* img1, const double* img2, const double* taps, int window_size, int B, int C, int H, int W, double* out,
                      double* means, ebos_stream_t stream) {
  return ebos::ssim_map_launch<double>("ebos_ssim_map_f64", img1, img2, taps, window_size, B, C, H, W, out, means, ebos::as_stream(stream));
}

int ebos_photometric_max_window(void) { return ebos::kPhMaxWindow; }

size_t ebos_ssim_means_elems(int dtype, int B, int C, int H, int W) {
  const int64_t N = (int64_t)B * C;
  if ((dtype != EBOS_IMAGE_F32 && dtype != EBOS_IMAGE_F64) || B <= 0 || C <= 0 || N > 65535 || !ebos::ph_shape_ok((int)N, H, W)) return 0;
  return (size_t)(N + B + 1) + 2 * (size_t)N * (1 + (size_t)ebos::ph_tiles(dtype, H, W));
}

size_t ebos_photometric_scratch_bytes(int dtype, int B, int H, int W) {
  if ((dtype != EBOS_IMAGE_F32 && dtype != EBOS_IMAGE_F64) || !ebos::ph_shape_ok(B, H, W)) return 0;
  return (size_t)B * (size_t)ebos::ph_tiles(dtype, H, W) * sizeof(ebos::PhPartial);
}

int ebos_photometric_batch(int dtype, int frame_dtype, int B, int H, int W, const void* frame1, int64_t frame1_sb, const void* frame2,
                           const void* flow, const void* taps, int window_size, int has_roi, int xmin, int xmax, int ymin, int ymax,
                           const uint8_t* mask, int64_t mask_sb, double* out, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(dtype == EBOS_IMAGE_F32 || dtype == EBOS_IMAGE_F64, "ebos_photometric_batch: dtype code %d is not built (%d = float32, %d = float64)",
               dtype, EBOS_IMAGE_F32, EBOS_IMAGE_F64);
  EBOS_REQUIRE(frame_dtype == EBOS_IMAGE_U8 || frame_dtype == dtype,
               "ebos_photometric_batch: frame dtype code %d is not built (%d = uint8, %d = the flow's type)", frame_dtype, EBOS_IMAGE_U8, dtype);
  EBOS_REQUIRE(ph_shape_ok(B, H, W), "ebos_photometric_batch: bad shape B = %d, H = %d, W = %d (1 <= B <= 65535, H, W >= 2, H W < 2^31)", B, H, W);
  EBOS_REQUIRE(ph_window_ok(window_size), "ebos_photometric_batch: window_size %d is not a positive odd number", window_size);
  EBOS_REQUIRE(frame1 && frame2 && flow && taps && out && scratch, "ebos_photometric_batch: NULL buffer");
  EBOS_REQUIRE(frame1_sb == 0 || frame1_sb >= (int64_t)H * W, "ebos_photometric_batch: frame1_sb %lld is neither 0 nor >= H W", (long long)frame1_sb);
  EBOS_REQUIRE(!mask || mask_sb == 0 || mask_sb >= (int64_t)H * W, "ebos_photometric_batch: mask_sb %lld is neither 0 nor >= H W", (long long)mask_sb);
  EBOS_REQUIRE(!has_roi || (xmin <= xmax && ymin <= ymax), "ebos_photometric_batch: roi rows [%d, %d) columns [%d, %d) is out of order", xmin,
               xmax, ymin, ymax);
  if (window_size > kPhMaxWindow) {
    set_error("ebos_photometric_batch: window_size %d > %d is not built", window_size, kPhMaxWindow);
    return EBOS_ERR_UNSUPPORTED;
  }
  const size_t need = ebos_photometric_scratch_bytes(dtype, B, H, W);
  if (scratch_bytes < need) {
    set_error("ebos_photometric_batch: scratch too small (%zu < %zu)", scratch_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  PhArgs a;
  a.frame1 = frame1;
  a.frame2 = frame2;
  a.flow = flow;
  a.taps = taps;
  a.mask = mask;
  a.frame1_sb = frame1_sb;
  a.mask_sb = mask_sb;
  a.ws = window_size;
  a.H = H;
  a.W = W;
  a.tiles_x = dtype == EBOS_IMAGE_F64 ? ph_tiles_x<double>(W) : ph_tiles_x<float>(W);
  a.tiles = ph_tiles(dtype, H, W);
  a.xmin = has_roi ? xmin : 0;
  a.xmax = has_roi ? xmax : H;
  a.ymin = has_roi ? ymin : 0;
  a.ymax = has_roi ? ymax : W;
  PhPartial* part = static_cast<PhPartial*>(scratch);
  return dtype == EBOS_IMAGE_F64 ? photometric_launch<double>(a, frame_dtype, B, part, out, as_stream(stream))
                                 : photometric_launch<float>(a, frame_dtype, B, part, out, as_stream(stream));
}

}  // extern "C"
