// frame_warp.hip -- batched perspective warp of camera frames into the event view (reference: src/data_loader/ccs.py:373-396,
// ``cv2.warpPerspective(image, homography, (W, H))``, and the driver's ``validate_image`` crop, bos_event.py:25-39, fused in).
//
// The arithmetic is the classic fixed-point warpPerspective (OpenCV 4.5 - 4.10) as tests/_warp_ref.py restates it: the inverse
// matrix in double, per destination pixel three double multiply-adds from the origin column of its 16-row block, one double
// divide, round half to even, 5 fraction bits per axis, 15-bit weights (uint8) or float products (float32), constant border.
// Every product and sum is rounded on its own (fp contract off for the whole file) so kernel, restatement and a scalar host
// build agree bit for bit.
//
// One launch per batch: grid = (column groups, row groups, frame).  A lane produces kPix adjacent pixels of one row and stores
// them as one 4-byte (uint8) or 16-byte (float32) word where the destination is aligned for it.  No atomics, no scratch; a
// frame's bits do not depend on the batch it is in, a pixel's bits do not depend on the output rectangle.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

#include "remap_sample.h"

namespace ebos {
namespace {

constexpr int kPix = 4;          // adjacent output pixels per lane
constexpr int kBlockX = 64;      // lanes along a row: one wave covers 256 adjacent pixels
constexpr int kBlockY = 4;
constexpr int kMaxMats = 32;     // per-frame matrices travel as kernel arguments: frames per launch when they differ

template <int N>
struct WarpMats {
  double m[N][9];                // INVERSE maps (destination -> source): N = 1 shared by the batch, else one per frame of the launch
};

struct WarpArgs {
  const void* src;
  void* out;
  int64_t src_sb, src_sr, out_sb, out_sr;   // element strides; unit columns
  int Hs, Ws;
  int bw;                                    // block width of the coordinate walk
  int x_first, y_first, w, h;                // output rectangle in destination coordinates (columns, rows)
  int nearest;
  double border;
};

template <typename T>
__device__ __forceinline__ T warp_pixel(const T* __restrict__ src, int64_t sr, int Hs, int Ws, const double* m, int bw, int x, double m1y,
                                        double m4y, double m7y, bool nearest, T cval) {
  const int xb = (x / bw) * bw;
  const double x0 = (double)xb, x1 = (double)(x - xb);
  const double X0 = (m[0] * x0 + m1y) + m[2];
  const double Y0 = (m[3] * x0 + m4y) + m[5];
  const double W0 = (m[6] * x0 + m7y) + m[8];
  const double Wd = W0 + m[6] * x1;
  const double s = Wd != 0.0 ? (nearest ? 1.0 : (double)kInterTab) / Wd : 0.0;
  const int X = round_clamped((X0 + m[0] * x1) * s);
  const int Y = round_clamped((Y0 + m[3] * x1) * s);
  return sample_tap<T>(src, sr, Hs, Ws, X, Y, nearest, cval);
}

template <typename T, bool VEC, int NM>
__global__ __launch_bounds__(kBlockX* kBlockY) void warp_perspective_kernel(WarpArgs a, WarpMats<NM> mats) {
  const int b = blockIdx.z;
  const int col = (blockIdx.x * kBlockX + threadIdx.x) * kPix;   // first of this lane's columns inside the rectangle
  const int row = blockIdx.y * kBlockY + threadIdx.y;
  if (col >= a.w || row >= a.h) return;
  const double* m = mats.m[NM > 1 ? b : 0];
  const T* src = static_cast<const T*>(a.src) + (int64_t)b * a.src_sb;
  T* out = static_cast<T*>(a.out) + (int64_t)b * a.out_sb + (int64_t)row * a.out_sr + col;
  const double y = (double)(a.y_first + row);
  const double m1y = m[1] * y, m4y = m[4] * y, m7y = m[7] * y;
  const T cval = Px<T>::border(a.border);
  const bool nearest = a.nearest != 0;
  const int x = a.x_first + col;
  if (col + kPix <= a.w) {
    T v[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) v[k] = warp_pixel<T>(src, a.src_sr, a.Hs, a.Ws, m, a.bw, x + k, m1y, m4y, m7y, nearest, cval);
    if (VEC) {
      *reinterpret_cast<typename Px<T>::vec*>(out) = Px<T>::pack(v);
    } else {
#pragma unroll
      for (int k = 0; k < kPix; ++k) out[k] = v[k];
    }
  } else {
    for (int k = 0; col + k < a.w; ++k) out[k] = warp_pixel<T>(src, a.src_sr, a.Hs, a.Ws, m, a.bw, x + k, m1y, m4y, m7y, nearest, cval);
  }
}

// one matrix of the call as the kernel takes it: checked, inverted unless the caller's is the inverse map already
bool inverse_map(const double* s, int flags, double* t) {
  for (int k = 0; k < 9; ++k)
    if (!isfinite(s[k]) || fabs(s[k]) > 1e100) return false;
  if (!(flags & EBOS_WARP_INVERSE_MAP)) return invert3x3(s, t);
  for (int k = 0; k < 9; ++k) t[k] = s[k];
  return true;
}

template <typename T, int NM>
int launch(const WarpArgs& a0, const double* M, int flags, int B, hipStream_t stream) {
  constexpr size_t kAlign = sizeof(typename Px<T>::vec);
  const bool vec = reinterpret_cast<uintptr_t>(a0.out) % kAlign == 0 && (a0.out_sb * sizeof(T)) % kAlign == 0 &&
                   (a0.out_sr * sizeof(T)) % kAlign == 0;
  const dim3 block(kBlockX, kBlockY, 1);
  const int per_launch = NM > 1 ? NM : 65535;
  for (int b0 = 0; b0 < B; b0 += per_launch) {
    const int nb = B - b0 < per_launch ? B - b0 : per_launch;
    WarpArgs a = a0;
    a.src = static_cast<const T*>(a0.src) + (int64_t)b0 * a0.src_sb;
    a.out = static_cast<T*>(a0.out) + (int64_t)b0 * a0.out_sb;
    WarpMats<NM> mats = {};
    for (int i = 0; i < (NM > 1 ? nb : 1); ++i) inverse_map(M + (NM > 1 ? (int64_t)(b0 + i) * 9 : 0), flags, mats.m[i]);
    const dim3 grid((a.w + kBlockX * kPix - 1) / (kBlockX * kPix), (a.h + kBlockY - 1) / kBlockY, nb);
    if (vec)
      hipLaunchKernelGGL((warp_perspective_kernel<T, true, NM>), grid, block, 0, stream, a, mats);
    else
      hipLaunchKernelGGL((warp_perspective_kernel<T, false, NM>), grid, block, 0, stream, a, mats);
    EBOS_CHECK_LAUNCH("ebos_warp_perspective: warp_perspective_kernel");
  }
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

using namespace ebos;

extern "C" {

int ebos_warp_perspective(int dtype, int B, int Hs, int Ws, const void* src, int64_t src_sb, int64_t src_sr, const double* M,
                          int64_t m_stride, int H, int W, int flags, double border_value, int xmin, int xmax, int ymin, int ymax,
                          void* out, int64_t out_sb, int64_t out_sr, ebos_stream_t stream) {
  EBOS_REQUIRE(dtype == EBOS_WARP_U8 || dtype == EBOS_WARP_F32, "ebos_warp_perspective: dtype %d is not U8 (0) or F32 (1)", dtype);
  EBOS_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "ebos_warp_perspective: bad shape B = %d, source %d x %d, destination %d x %d",
               B, Hs, Ws, H, W);
  EBOS_REQUIRE(Hs <= 32767 && Ws <= 32767, "ebos_warp_perspective: source %d x %d exceeds the int16 coordinates of the algorithm", Hs, Ws);
  EBOS_REQUIRE(H <= 65535 && W <= 65535, "ebos_warp_perspective: destination %d x %d too large", H, W);
  EBOS_REQUIRE(src && out && M, "ebos_warp_perspective: NULL buffer");
  EBOS_REQUIRE(src_sb >= 0 && src_sr >= Ws && out_sb >= 0 && out_sr >= 0, "ebos_warp_perspective: bad strides");
  EBOS_REQUIRE(m_stride == 0 || m_stride == 9, "ebos_warp_perspective: matrix stride %lld is neither 0 (shared) nor 9", (long long)m_stride);
  EBOS_REQUIRE(0 <= xmin && xmin < xmax && xmax <= H && 0 <= ymin && ymin < ymax && ymax <= W,
               "ebos_warp_perspective: rectangle rows [%d, %d) columns [%d, %d) outside the %d x %d destination", xmin, xmax, ymin, ymax, H, W);
  EBOS_REQUIRE(out_sr >= ymax - ymin, "ebos_warp_perspective: output row stride %lld < %d columns", (long long)out_sr, ymax - ymin);
  EBOS_REQUIRE(isfinite(border_value), "ebos_warp_perspective: border value is not finite");
  const int interp = flags & ~EBOS_WARP_INVERSE_MAP;
  if (interp != EBOS_WARP_INTER_NEAREST && interp != EBOS_WARP_INTER_LINEAR) {
    set_error("ebos_warp_perspective: flags %d: only INTER_NEAREST (0), INTER_LINEAR (1) and WARP_INVERSE_MAP (16) are supported", flags);
    return EBOS_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < (m_stride ? B : 1); ++i) {   // every matrix is checked before anything is launched
    double t[9];
    if (!inverse_map(M + (int64_t)i * 9, flags, t)) {
      set_error("ebos_warp_perspective: matrix %d is singular, not finite or beyond 1e100", i);
      return EBOS_ERR_INVALID_ARG;
    }
  }
  WarpArgs a;
  a.src = src;
  a.out = out;
  a.src_sb = src_sb;
  a.src_sr = src_sr;
  a.out_sb = out_sb;
  a.out_sr = out_sr;
  a.Hs = Hs;
  a.Ws = Ws;
  const int bh = H < 16 ? H : 16;
  a.bw = 1024 / bh < W ? 1024 / bh : W;
  a.x_first = ymin;
  a.y_first = xmin;
  a.w = ymax - ymin;
  a.h = xmax - xmin;
  a.nearest = interp == EBOS_WARP_INTER_NEAREST;
  a.border = border_value;
  const hipStream_t st = as_stream(stream);
  if (dtype == EBOS_WARP_U8) return m_stride ? launch<uint8_t, kMaxMats>(a, M, flags, B, st) : launch<uint8_t, 1>(a, M, flags, B, st);
  return m_stride ? launch<float, kMaxMats>(a, M, flags, B, st) : launch<float, 1>(a, M, flags, B, st);
}

}  // extern "C"
