// warp_footprint.h -- what the general and LDS-tiled event kernels share around one bilinear vote: the warped footprint of an event,
// the accumulator type of an LDS tile window and the upstream image of the backwards.  Included by iwe_fused.hip (one reference
// time), iwe_multiref.hip (K reference times) and warp_voxel_core.h (the time-aware warp).  The slab pipeline (iwe_tile_core.h)
// keeps its own: its warped_taps takes the decoded source pixel.
#pragma once
#include <type_traits>

#include "common.h"

namespace ebos {
namespace {

constexpr float kEps = 1e-6f;  // src/event_image_converter.py:586

// Warped footprint in SOURCE-PIXEL-RELATIVE coordinates.  x' = x + d with d = -dt * u.  Writing
// x = rs + fx (rs = trunc(x), fx exact) gives floor(x' + eps) = rs + floor(fx + d + eps): the float
// arithmetic only ever sees |fx + d| <~ 32, so its rounding error is ~2e-6 px instead of the ~1e-4 px
// of absolute 1280-px coordinates.  That matters because the bilinear splat's derivative jumps at
// integer coordinates: every event rounded across an integer flips its gradient contribution.
struct Taps {
  int R, C;      // top-left tap, padded image coordinates
  float fr, fc;  // fractional offsets
  bool ok;       // finite
};
__device__ __forceinline__ Taps warped_taps(float ex, float ey, float dx, float dy, int pad_h, int pad_w) {
  const int rs = (int)ex, cs = (int)ey;
  const float lx = (ex - (float)rs) + dx, ly = (ey - (float)cs) + dy;
  const float r0 = floorf(lx + kEps), c0 = floorf(ly + kEps);
  Taps t;
  t.fr = lx - r0;
  t.fc = ly - c0;
  t.ok = (r0 > -1e9f) && (r0 < 1e9f) && (c0 > -1e9f) && (c0 < 1e9f);
  t.R = t.ok ? rs + (int)r0 + pad_h : -4;
  t.C = t.ok ? cs + (int)c0 + pad_w : -4;
  return t;
}

template <int TH, int TW, int HALO>
struct TileAcc {  // f64 when it fits the LDS, else f32
  static constexpr bool kF64 = (size_t)(TH + 2 * HALO) * (TW + 2 * HALO) * sizeof(double) <= 160 * 1024;
  using type = typename std::conditional<kF64, double, float>::type;
};

struct GradImage {
  const float* g;
  float a, c;  // G = a * g + c inside the valid region
  int h, w, lo;
  __device__ __forceinline__ float at(int R, int C) const {
    if (R < lo || R >= h - lo || C < lo || C >= w - lo) return 0.0f;
    return a * g[(int64_t)R * w + C] + c;
  }
};

}  // namespace
}  // namespace ebos
