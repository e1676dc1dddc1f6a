// image_warp.h -- the coordinate chain of the reference's warp_image_forward / warp_image_torch (src/utils/frame_utils.py:56-115)
// and grid_sample's bilinear taps (mode="bilinear", padding_mode="zeros", align_corners=True), every operation rounded on its own
// (the including file is compiled without FMA contraction):
//   base  = i / ((size - 1) / 2) - 1            in float32: torch divides an integer tensor by a Python float in its default dtype
//   wn    = base - flow / ((size - 1) / 2)      in the type of the flow
//   pos   = (wn + 1) * ((size - 1) / 2)         grid_sample's un-normalisation, in the type of the sampled image
//   taps at floor(pos) and floor(pos) + 1, weights (1 - frac, frac) per axis, zeros outside the image
//   out   = fma(se, n w, fma(sw, n e, fma(ne, s w, nw * (s e)))): torch's CPU grid_sample adds the four products from the left with
//           each multiply-add fused (its x86 builds contract them; the reference's float32 and float64 outputs are reproduced bit
//           for bit by exactly this pattern and by no unfused one) -- three explicit fma calls, the only fused operations here
// csrc/gml.hip keeps its own copy of this chain inside warp_at (float64 only, with the derivatives by the flow next to it, the
// four products added unfused).
#pragma once
#include "common.h"

namespace ebos {

// the normalised coordinate of pixel index i on an axis of `size` pixels, displaced by `flow` pixels
template <typename T>
__device__ __forceinline__ T warp_normalised(int i, int size, T flow) {
  const double k = (size - 1) / 2.0;
  const float base = (float)i / (float)k - 1.0f;
  return (T)base - flow / (T)k;
}

// the same in float32 with the displacement already divided by (size - 1) / 2 (warp_image_torch: a 0-dim shift leaves the grid float32)
__device__ __forceinline__ float warp_normalised_f32(int i, int size, float q) {
  const double k = (size - 1) / 2.0;
  return ((float)i / (float)k - 1.0f) - q;
}

template <typename T>
__device__ __forceinline__ T warp_unnormalise(T wn, int size) {
  return (wn + T(1)) * (T)((size - 1) / 2.0);
}

template <typename T>
struct WarpTaps {
  int y0, x0;     // the north-west tap (meaningful when `near`)
  T n, s, w, e;   // weights of the lower / upper row and of the right / left column
  bool near;      // some tap may lie inside the image (false for NaN / inf / far-away positions)
  bool inside;    // all four taps lie inside the image
};

template <typename T>
__device__ __forceinline__ WarpTaps<T> warp_taps(T iy, T ix, int H, int W) {
  WarpTaps<T> t;
  const T fy = floor(iy), fx = floor(ix);
  t.n = iy - fy;
  t.s = T(1) - t.n;
  t.w = ix - fx;
  t.e = T(1) - t.w;
  t.near = fy > T(-2) && fy < (T)H && fx > T(-2) && fx < (T)W;
  t.y0 = t.near ? (int)fy : -2;
  t.x0 = t.near ? (int)fx : -2;
  t.inside = t.near && t.y0 >= 0 && t.y0 + 1 < H && t.x0 >= 0 && t.x0 + 1 < W;
  return t;
}

// the bilinear sample of img [H, W] (element type IT, converted to T) at the taps; a non-finite position gives NaN, as torch's does
template <typename T, typename IT>
__device__ __forceinline__ T warp_gather(const IT* __restrict__ img, int H, int W, const WarpTaps<T>& t) {
  T a[4] = {T(0), T(0), T(0), T(0)};   // nw, ne, sw, se
  if (t.near) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int y = t.y0 + i, x = t.x0 + j;
        if (y >= 0 && y < H && x >= 0 && x < W) a[i * 2 + j] = (T)img[(size_t)y * W + x];
      }
  }
  T v = a[0] * (t.s * t.e);
  v = __builtin_elementwise_fma(a[1], t.s * t.w, v);
  v = __builtin_elementwise_fma(a[2], t.n * t.e, v);
  return __builtin_elementwise_fma(a[3], t.n * t.w, v);
}

}  // namespace ebos
