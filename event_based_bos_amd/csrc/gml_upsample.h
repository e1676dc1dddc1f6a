// gml_upsample.h -- the float64 patch -> dense upsample of the generative solvers, one axis at a time: shared by the Adam loops
// (gml.hip) and the sweep's flow scatter (eklt_sweep.hip), so that both evaluate the map with the same operations.
//
// upsampled index o = r + off; source coordinate max((o + 0.5) / s - 0.5, 0) on the (g + 2k)-cell padded axis; padded cell i
// is grid cell clamp(i - k, 0, g - 1).  (torch's upsample_bilinear2d, align_corners=False, scale = 1 / s.)  The pyramid has
// s = p, k = 1.
#pragma once
#include "common.h"

namespace ebos {

struct Tap {
  int c0, c1;
  double l0, l1;
};

__device__ __forceinline__ Tap up_tap(int r, int off, int s, int k, int g) {
#pragma clang fp contract(off)
  const double scale = 1.0 / (double)s;
  double src = scale * ((double)(r + off) + 0.5) - 0.5;
  if (src < 0.0) src = 0.0;
  int i0 = (int)src;
  const int padded = g + 2 * k;
  const int i1 = i0 + ((i0 < padded - 1) ? 1 : 0);
  double l1 = src - (double)i0;
  l1 = l1 < 0.0 ? 0.0 : (l1 > 1.0 ? 1.0 : l1);
  Tap t;
  t.l1 = l1;
  t.l0 = 1.0 - l1;
  t.c0 = min(max(i0 - k, 0), g - 1);
  t.c1 = min(max(i1 - k, 0), g - 1);
  return t;
}

__device__ __forceinline__ double up_eval(const double* __restrict__ grid, int gw, const Tap& tr, const Tap& tc) {
#pragma clang fp contract(off)
  const double v00 = grid[tr.c0 * gw + tc.c0], v01 = grid[tr.c0 * gw + tc.c1];
  const double v10 = grid[tr.c1 * gw + tc.c0], v11 = grid[tr.c1 * gw + tc.c1];
  return tr.l0 * (tc.l0 * v00 + tc.l1 * v01) + tr.l1 * (tc.l0 * v10 + tc.l1 * v11);
}

}  // namespace ebos
