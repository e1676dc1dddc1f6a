// remap_sample.h -- the sampling half of the classic fixed-point remap, shared by frame_warp.hip (perspective warp) and rectify.hip
// (lens rectification): a source coordinate scaled by 32 and rounded (5 fraction bits per axis) -> one destination pixel, with
// 15-bit weights (uint8) or float products (float32) and a constant border.  tests/_warp_ref.py restates it in numpy.
// Every product and sum is rounded on its own: the including file compiles with fp contraction off.
#pragma once
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace ebos {

constexpr int kInterBits = 5;
constexpr int kInterTab = 1 << kInterBits;

template <typename T>
struct Px;
template <>
struct Px<uint8_t> {
  using vec = uint32_t;
  static __device__ __forceinline__ uint8_t border(double v) {
    const double r = rint(v);
    return (uint8_t)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
  }
  static __device__ __forceinline__ uint8_t blend(uint8_t s00, uint8_t s01, uint8_t s10, uint8_t s11, int fx, int fy) {
    // the 32 x 32 table of the restatement in closed form: 32768 (1 - fy / 32)(1 - fx / 32) = 32 (32 - fy)(32 - fx), ...
    const int ax = kInterTab - fx, ay = kInterTab - fy;
    const int acc = (int)s00 * (32 * ay * ax) + (int)s01 * (32 * ay * fx) + (int)s10 * (32 * fy * ax) + (int)s11 * (32 * fy * fx);
    return (uint8_t)((acc + (1 << 14)) >> 15);
  }
  static __device__ __forceinline__ vec pack(const uint8_t* v) {
    return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  }
};
template <>
struct Px<float> {
  using vec = float4;
  static __device__ __forceinline__ float border(double v) { return (float)v; }
  static __device__ __forceinline__ float blend(float s00, float s01, float s10, float s11, int fx, int fy) {
    const float step = 1.0f / kInterTab;
    const float bx = (float)fx * step, by = (float)fy * step;
    const float ax = 1.0f - bx, ay = 1.0f - by;
    return ((s00 * (ay * ax) + s01 * (ay * bx)) + s10 * (by * ax)) + s11 * (by * bx);
  }
  static __device__ __forceinline__ vec pack(const float* v) { return make_float4(v[0], v[1], v[2], v[3]); }
};

// (fmin / fmax return the other operand for a NaN, as numpy's fmin / fmax do in the restatement: a NaN coordinate -- inf * 0 where
// 32 / W overflows -- becomes INT_MAX in both, which is outside every source)
__device__ __forceinline__ int round_clamped(double v) {
  v = fmax(-2147483648.0, fmin(2147483647.0, v));
  return (int)rint(v);
}
__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// the pixel at the rounded source coordinate (X, Y): whole pixels for `nearest`, else scaled by 32; taps outside the source are cval
template <typename T>
__device__ __forceinline__ T sample_tap(const T* __restrict__ src, int64_t sr, int Hs, int Ws, int X, int Y, bool nearest, T cval) {
  if (nearest) {
    const int sx = sat16(X), sy = sat16(Y);
    return ((unsigned)sx < (unsigned)Ws && (unsigned)sy < (unsigned)Hs) ? src[(int64_t)sy * sr + sx] : cval;
  }
  const int sx = sat16(X >> kInterBits), sy = sat16(Y >> kInterBits);
  const int fx = X & (kInterTab - 1), fy = Y & (kInterTab - 1);
  const bool c0 = (unsigned)sx < (unsigned)Ws, c1 = (unsigned)(sx + 1) < (unsigned)Ws;
  const bool r0 = (unsigned)sy < (unsigned)Hs, r1 = (unsigned)(sy + 1) < (unsigned)Hs;
  if (!((c0 || c1) && (r0 || r1))) return cval;
  const T* p = src + (int64_t)sy * sr + sx;
  const T s00 = (r0 && c0) ? p[0] : cval;
  const T s01 = (r0 && c1) ? p[1] : cval;
  const T s10 = (r1 && c0) ? p[sr] : cval;
  const T s11 = (r1 && c1) ? p[sr + 1] : cval;
  return Px<T>::blend(s00, s01, s10, s11, fx, fy);
}

// closed-form inverse: cofactors times ONE reciprocal of the determinant (false: singular or not finite)
inline bool invert3x3(const double* s, double* t) {
  const double det = s[0] * (s[4] * s[8] - s[5] * s[7]) - s[1] * (s[3] * s[8] - s[5] * s[6]) + s[2] * (s[3] * s[7] - s[4] * s[6]);
  if (det == 0.0 || !isfinite(det)) return false;
  const double d = 1.0 / det;
  t[0] = (s[4] * s[8] - s[5] * s[7]) * d;
  t[1] = (s[2] * s[7] - s[1] * s[8]) * d;
  t[2] = (s[1] * s[5] - s[2] * s[4]) * d;
  t[3] = (s[5] * s[6] - s[3] * s[8]) * d;
  t[4] = (s[0] * s[8] - s[2] * s[6]) * d;
  t[5] = (s[2] * s[3] - s[0] * s[5]) * d;
  t[6] = (s[3] * s[7] - s[4] * s[6]) * d;
  t[7] = (s[1] * s[6] - s[0] * s[7]) * d;
  t[8] = (s[0] * s[4] - s[1] * s[3]) * d;
  for (int i = 0; i < 9; ++i)
    if (!isfinite(t[i])) return false;
  return true;
}

}  // namespace ebos
