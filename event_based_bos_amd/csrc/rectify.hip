// rectify.hip -- lens calibration on the GPU: from a camera matrix K and OpenCV-order distortion coefficients D to rectified
// sub-pixel events and rectified frames (reference: src/utils/event_utils.py:242-266 ``undistort_events``, the loaders'
// ``load_calib`` / ``undistort``, src/solver/base.py:363-378 ``undistort_image``).
//
// The model, as tests/_rectify_ref.py restates it in numpy with the same operation order (fp contract off for the whole file, every
// product and sum rounded on its own):
//   r2 = x x + y y;  rad = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2);  a = (2 x) y
//   dx = p1 a + p2 (r2 + 2 (x x));  dy = p1 (r2 + 2 (y y)) + p2 a;  u = fx (x rad + dx) + cx;  v = fy (y rad + dy) + cy
// and its inverse by a FIXED number of fixed-point steps x = (x0 - dx(x, y)) / rad(x, y), y likewise, from (x0, y0).
//
//   ebos_rectify_map_f64      one thread per sensor pixel runs the inverse: [H, W, 2] = (row', col') under new_K.  Plain stores.
//   ebos_rectify_events_raw   raw columns + that map -> [m, 4] events in stream order: keep flag, the device-wide exclusive scan of
//                             event_plan.hip (scan_exclusive_i32, as ebos_filter_compact uses it), scatter.  Per event a coalesced
//                             13 B read, one 16 B gather from the map, a 32 B (float64) row store.
//   ebos_undistort_events_*   the reference's undistort_events on an [n, 4] array, through the same compaction.
//   ebos_undistort_image_*    per output pixel: ideal position (through an inverse homography where given) -> normalise by new_K
//                             -> forward model -> the fixed-point sampling of remap_sample.h.  One resample for "undistort, then
//                             warp into the event view".  With D = 0 and new_K = K the lens step is skipped and the coordinate
//                             chain is the perspective kernel's (frame_warp.hip), bit for bit.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

#include "remap_sample.h"

namespace ebos {
namespace {

constexpr int kBlock = 256;
constexpr int kPix = 4;          // adjacent output pixels per lane (images)
constexpr int kBlockX = 64;
constexpr int kBlockY = 4;

struct Camera {
  double fx, fy, cx, cy;         // K
  double nfx, nfy, ncx, ncy;     // new_K
  double k1, k2, p1, p2, k3, k4, k5, k6;
};

Camera camera_of(const double* c) {
  Camera k;
  k.fx = c[0], k.fy = c[1], k.cx = c[2], k.cy = c[3];
  k.nfx = c[4], k.nfy = c[5], k.ncx = c[6], k.ncy = c[7];
  k.k1 = c[8], k.k2 = c[9], k.p1 = c[10], k.p2 = c[11], k.k3 = c[12], k.k4 = c[13], k.k5 = c[14], k.k6 = c[15];
  return k;
}

bool camera_ok(const double* c) {
  for (int i = 0; i < 16; ++i)
    if (!isfinite(c[i])) return false;
  return c[0] != 0.0 && c[1] != 0.0 && c[4] != 0.0 && c[5] != 0.0;
}

bool camera_has_lens(const double* c) {
  for (int i = 8; i < 16; ++i)
    if (c[i] != 0.0) return true;
  for (int i = 0; i < 4; ++i)
    if (c[i] != c[4 + i]) return true;
  return false;
}

__device__ __forceinline__ void lens_terms(const Camera& k, double x, double y, double* rad, double* dx, double* dy) {
  const double xx = x * x, yy = y * y;
  const double r2 = xx + yy;
  const double num = 1.0 + ((k.k3 * r2 + k.k2) * r2 + k.k1) * r2;
  const double den = 1.0 + ((k.k6 * r2 + k.k5) * r2 + k.k4) * r2;
  *rad = num / den;
  const double a = (2.0 * x) * y;
  *dx = k.p1 * a + k.p2 * (r2 + 2.0 * xx);
  *dy = k.p1 * (r2 + 2.0 * yy) + k.p2 * a;
}

// ---- the map -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void rectify_map_kernel(Camera k, int iterations, int H, int W, double2* __restrict__ map) {
  const int64_t P = (int64_t)H * W;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
    const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
    const double x0 = ((double)c - k.cx) / k.fx, y0 = ((double)r - k.cy) / k.fy;
    double x = x0, y = y0;
    for (int it = 0; it < iterations; ++it) {
      double rad, dx, dy;
      lens_terms(k, x, y, &rad, &dx, &dy);
      x = (x0 - dx) / rad;
      y = (y0 - dy) / rad;
    }
    map[i] = make_double2(k.nfy * y + k.ncy, k.nfx * x + k.ncx);   // (row', col')
  }
}

// ---- events ------------------------------------------------------------------------------------------------------------------
struct RawArgs {
  const int16_t* col;
  const int16_t* row;
  const void* t;
  const uint8_t* pol;
  const double2* map;
  int64_t n;
  double ticks;
  int t64;
  int H, W, H_out, W_out;
};

template <typename T>
struct Row4;
template <>
struct Row4<double> {
  static __device__ __forceinline__ void store(double* p, double a, double b, double c, double d) {
    reinterpret_cast<double2*>(p)[0] = make_double2(a, b);
    reinterpret_cast<double2*>(p)[1] = make_double2(c, d);
  }
};
template <>
struct Row4<float> {
  static __device__ __forceinline__ void store(float* p, float a, float b, float c, float d) {
    *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
  }
};

// the rectified position of event i in the output's element type; false: dropped (*outside_sensor says by which rule)
template <typename T>
__device__ __forceinline__ bool rectified(const RawArgs& a, int64_t i, T* x, T* y, bool* outside_sensor) {
  const int c = a.col[i], r = a.row[i];
  *outside_sensor = !((unsigned)c < (unsigned)a.W && (unsigned)r < (unsigned)a.H);
  if (*outside_sensor) return false;                     // the map is never read out of bounds
  const double2 m = a.map[(int64_t)r * a.W + c];
  *x = (T)m.x;
  *y = (T)m.y;
  return *x >= T(0) && *x < (T)a.H_out && *y >= T(0) && *y < (T)a.W_out;   // (a NaN fails every comparison)
}

template <typename T>
__global__ __launch_bounds__(kBlock) void rectify_flag_kernel(RawArgs a, int32_t* __restrict__ keep, int32_t* n_outside_sensor) {
  int32_t outside = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
    T x, y;
    bool os;
    keep[i] = rectified<T>(a, i, &x, &y, &os) ? 1 : 0;
    outside += os ? 1 : 0;
  }
  outside = wave_sum(outside);                            // an integer count: its value does not depend on the order of the adds
  if ((threadIdx.x & (kWave - 1)) == 0 && outside) atomicAdd(n_outside_sensor, outside);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void rectify_scatter_kernel(RawArgs a, const int32_t* __restrict__ offset, T* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
    T x, y;
    bool os;
    if (!rectified<T>(a, i, &x, &y, &os)) continue;
    const double ticks = a.t64 ? (double)static_cast<const int64_t*>(a.t)[i] : (double)static_cast<const int32_t*>(a.t)[i];
    Row4<T>::store(out + (int64_t)offset[i] * 4, x, y, (T)(ticks / a.ticks), a.pol[i] ? T(1) : T(0));
  }
}

// ---- undistort_events --------------------------------------------------------------------------------------------------------
struct UndistArgs {
  const void* events;
  const double* map_x;
  const double* map_y;
  int64_t n;
  int mh, mw, h, w;
};

// numpy's astype(int32) of a float followed by numpy's indexing: truncation toward zero, negative indices count from the end;
// false where numpy raises IndexError (or the value is not an int32)
__device__ __forceinline__ bool numpy_index(double v, int size, int* idx) {
  if (!(v > -2147483649.0 && v < 2147483648.0)) return false;
  int i = (int)v;
  if (i < 0) i += size;
  *idx = i;
  return (unsigned)i < (unsigned)size;
}
__device__ __forceinline__ int to_i32(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT32_MIN; }

template <typename T>
__device__ __forceinline__ bool undistorted(const UndistArgs& a, int64_t i, int* k, int* l, bool* bad_index) {
  const T* e = static_cast<const T*>(a.events) + i * 4;
  int ix, iy;
  *bad_index = !(numpy_index((double)e[0], a.mh, &ix) && numpy_index((double)e[1], a.mw, &iy));
  if (*bad_index) return false;
  *k = to_i32(a.map_y[(int64_t)ix * a.mw + iy]);
  *l = to_i32(a.map_x[(int64_t)ix * a.mw + iy]);
  return 0 <= *k && *k < a.h && 0 <= *l && *l < a.w;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void undistort_flag_kernel(UndistArgs a, int32_t* __restrict__ keep, int32_t* n_bad_index) {
  int32_t bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
    int k, l;
    bool b;
    keep[i] = undistorted<T>(a, i, &k, &l, &b) ? 1 : 0;
    bad += b ? 1 : 0;
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & (kWave - 1)) == 0 && bad) atomicAdd(n_bad_index, bad);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void undistort_scatter_kernel(UndistArgs a, const int32_t* __restrict__ offset, T* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
    int k, l;
    bool b;
    if (!undistorted<T>(a, i, &k, &l, &b)) continue;
    const T* e = static_cast<const T*>(a.events) + i * 4;
    Row4<T>::store(out + (int64_t)offset[i] * 4, (T)k, (T)l, e[2], e[3]);
  }
}

struct Scratch {
  int32_t* keep;         // n: keep flags, then their exclusive scan
  int32_t* block_sums;   // scan_blocks(n)
};
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
Scratch carve(void* scratch, int64_t n) {
  Scratch s;
  s.keep = static_cast<int32_t*>(scratch);
  s.block_sums = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + align256((size_t)(n > 0 ? n : 1) * 4));
  return s;
}

template <typename T>
int undistort_events(const void* events, int64_t n, const double* map_x, const double* map_y, int mh, int mw, int h, int w, void* out,
                     int32_t* counts, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(n >= 0 && n <= EBOS_RECTIFY_MAX_EVENTS, "ebos_undistort_events: n = %lld outside 0 .. %lld", (long long)n,
               (long long)EBOS_RECTIFY_MAX_EVENTS);
  EBOS_REQUIRE(mh > 0 && mw > 0 && h >= 0 && w >= 0, "ebos_undistort_events: bad shape, maps %d x %d, image %d x %d", mh, mw, h, w);
  EBOS_REQUIRE(counts && ((events && out && map_x && map_y && scratch) || n == 0), "ebos_undistort_events: NULL buffer");
  EBOS_REQUIRE(reinterpret_cast<uintptr_t>(events) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
               "ebos_undistort_events: events and out must be 16-byte aligned");
  if (scratch_bytes < ebos_rectify_scratch_bytes(n)) {
    set_error("ebos_undistort_events: scratch too small (%zu < %zu)", scratch_bytes, ebos_rectify_scratch_bytes(n));
    return EBOS_ERR_SCRATCH;
  }
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(counts, 0, 8, s) != hipSuccess) {
    set_error("ebos_undistort_events: hipMemsetAsync failed");
    return EBOS_ERR_LAUNCH;
  }
  if (n == 0) return EBOS_OK;
  UndistArgs a = {events, map_x, map_y, n, mh, mw, h, w};
  Scratch sc = carve(scratch, n);
  const dim3 blk(kBlock), g(stream_grid(n, kBlock));
  undistort_flag_kernel<T><<<g, blk, 0, s>>>(a, sc.keep, counts + 1);
  scan_exclusive_i32(sc.keep, n, counts, sc.block_sums, s);
  undistort_scatter_kernel<T><<<g, blk, 0, s>>>(a, sc.keep, static_cast<T*>(out));
  EBOS_CHECK_LAUNCH("ebos_undistort_events");
  return EBOS_OK;
}

// ---- images ------------------------------------------------------------------------------------------------------------------
struct ImageArgs {
  const void* src;
  void* out;
  int64_t src_sb, src_sr, out_sb, out_sr;   // element strides; unit columns
  int Hs, Ws;
  int bw;                                    // block width of the coordinate walk (the perspective kernel's)
  int x_first, y_first, w, h;                // output rectangle in destination coordinates (columns, rows)
  int lens;                                  // 0: D = 0 and new_K = K -- the perspective kernel's chain alone
  double border;
  double m[9];                               // INVERSE homography (destination -> ideal frame); the identity without one
  Camera cam;
};

template <typename T>
__device__ __forceinline__ T rectify_pixel(const T* __restrict__ src, const ImageArgs& a, int x, double m1y, double m4y, double m7y, T cval) {
  const double* m = a.m;
  const int xb = (x / a.bw) * a.bw;
  const double x0 = (double)xb, x1 = (double)(x - xb);
  const double X0 = (m[0] * x0 + m1y) + m[2];
  const double Y0 = (m[3] * x0 + m4y) + m[5];
  const double W0 = (m[6] * x0 + m7y) + m[8];
  const double Wd = W0 + m[6] * x1;
  int X, Y;
  if (!a.lens) {
    const double s = Wd != 0.0 ? (double)kInterTab / Wd : 0.0;
    X = round_clamped((X0 + m[0] * x1) * s);
    Y = round_clamped((Y0 + m[3] * x1) * s);
  } else {
    const double s = Wd != 0.0 ? 1.0 / Wd : 0.0;
    const double xn = ((X0 + m[0] * x1) * s - a.cam.ncx) / a.cam.nfx;
    const double yn = ((Y0 + m[3] * x1) * s - a.cam.ncy) / a.cam.nfy;
    double rad, dx, dy;
    lens_terms(a.cam, xn, yn, &rad, &dx, &dy);
    const double u = a.cam.fx * (xn * rad + dx) + a.cam.cx;
    const double v = a.cam.fy * (yn * rad + dy) + a.cam.cy;
    X = round_clamped(u * (double)kInterTab);
    Y = round_clamped(v * (double)kInterTab);
  }
  return sample_tap<T>(src, a.src_sr, a.Hs, a.Ws, X, Y, false, cval);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlockX* kBlockY) void undistort_image_kernel(ImageArgs a) {
  const int b = blockIdx.z;
  const int col = (blockIdx.x * kBlockX + threadIdx.x) * kPix;   // first of this lane's columns inside the rectangle
  const int row = blockIdx.y * kBlockY + threadIdx.y;
  if (col >= a.w || row >= a.h) return;
  const T* src = static_cast<const T*>(a.src) + (int64_t)b * a.src_sb;
  T* out = static_cast<T*>(a.out) + (int64_t)b * a.out_sb + (int64_t)row * a.out_sr + col;
  const double y = (double)(a.y_first + row);
  const double m1y = a.m[1] * y, m4y = a.m[4] * y, m7y = a.m[7] * y;
  const T cval = Px<T>::border(a.border);
  const int x = a.x_first + col;
  if (col + kPix <= a.w) {
    T v[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) v[k] = rectify_pixel<T>(src, a, x + k, m1y, m4y, m7y, cval);
    if (VEC) {
      *reinterpret_cast<typename Px<T>::vec*>(out) = Px<T>::pack(v);
    } else {
#pragma unroll
      for (int k = 0; k < kPix; ++k) out[k] = v[k];
    }
  } else {
    for (int k = 0; col + k < a.w; ++k) out[k] = rectify_pixel<T>(src, a, x + k, m1y, m4y, m7y, cval);
  }
}

template <typename T>
int undistort_image(int B, int Hs, int Ws, const void* src, int64_t src_sb, int64_t src_sr, const double* cam, const double* M, int H, int W,
                    double border_value, int xmin, int xmax, int ymin, int ymax, void* out, int64_t out_sb, int64_t out_sr,
                    ebos_stream_t stream) {
  EBOS_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "ebos_undistort_image: bad shape B = %d, source %d x %d, destination %d x %d", B,
               Hs, Ws, H, W);
  EBOS_REQUIRE(Hs <= 32767 && Ws <= 32767, "ebos_undistort_image: source %d x %d exceeds the int16 coordinates of the algorithm", Hs, Ws);
  EBOS_REQUIRE(H <= 65535 && W <= 65535, "ebos_undistort_image: destination %d x %d too large", H, W);
  EBOS_REQUIRE(src && out && cam, "ebos_undistort_image: NULL buffer");
  EBOS_REQUIRE(src_sb >= 0 && src_sr >= Ws && out_sb >= 0 && out_sr >= 0, "ebos_undistort_image: bad strides");
  EBOS_REQUIRE(0 <= xmin && xmin < xmax && xmax <= H && 0 <= ymin && ymin < ymax && ymax <= W,
               "ebos_undistort_image: rectangle rows [%d, %d) columns [%d, %d) outside the %d x %d destination", xmin, xmax, ymin, ymax, H, W);
  EBOS_REQUIRE(out_sr >= ymax - ymin, "ebos_undistort_image: output row stride %lld < %d columns", (long long)out_sr, ymax - ymin);
  EBOS_REQUIRE(isfinite(border_value), "ebos_undistort_image: border value is not finite");
  EBOS_REQUIRE(camera_ok(cam), "ebos_undistort_image: the camera model is not finite or has a zero focal length");
  ImageArgs a;
  if (M) {
    bool ok = true;
    for (int k = 0; k < 9; ++k) ok = ok && isfinite(M[k]) && fabs(M[k]) <= 1e100;
    EBOS_REQUIRE(ok && invert3x3(M, a.m), "ebos_undistort_image: the homography is singular, not finite or beyond 1e100");
  } else {
    for (int k = 0; k < 9; ++k) a.m[k] = (k % 4 == 0) ? 1.0 : 0.0;
  }
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
  a.lens = camera_has_lens(cam) ? 1 : 0;
  a.border = border_value;
  a.cam = camera_of(cam);
  constexpr size_t kAlign = sizeof(typename Px<T>::vec);
  const bool vec = reinterpret_cast<uintptr_t>(out) % kAlign == 0 && (out_sb * sizeof(T)) % kAlign == 0 && (out_sr * sizeof(T)) % kAlign == 0;
  const dim3 block(kBlockX, kBlockY, 1);
  const hipStream_t st = as_stream(stream);
  for (int b0 = 0; b0 < B; b0 += 65535) {
    const int nb = B - b0 < 65535 ? B - b0 : 65535;
    ImageArgs ab = a;
    ab.src = static_cast<const T*>(src) + (int64_t)b0 * src_sb;
    ab.out = static_cast<T*>(out) + (int64_t)b0 * out_sb;
    const dim3 grid((a.w + kBlockX * kPix - 1) / (kBlockX * kPix), (a.h + kBlockY - 1) / kBlockY, nb);
    if (vec)
      hipLaunchKernelGGL((undistort_image_kernel<T, true>), grid, block, 0, st, ab);
    else
      hipLaunchKernelGGL((undistort_image_kernel<T, false>), grid, block, 0, st, ab);
    EBOS_CHECK_LAUNCH("ebos_undistort_image: undistort_image_kernel");
  }
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

using namespace ebos;

extern "C" {

int ebos_rectify_map_f64(const double* camera, int iterations, int H, int W, double* map, ebos_stream_t stream) {
  EBOS_REQUIRE(camera && map, "ebos_rectify_map_f64: NULL buffer");
  EBOS_REQUIRE(H > 0 && W > 0 && H <= 32767 && W <= 32767, "ebos_rectify_map_f64: sensor %d x %d outside 1 .. 32767 a side", H, W);
  EBOS_REQUIRE(iterations >= 1 && iterations <= 1000, "ebos_rectify_map_f64: iterations = %d outside 1 .. 1000", iterations);
  EBOS_REQUIRE(camera_ok(camera), "ebos_rectify_map_f64: the camera model is not finite or has a zero focal length");
  EBOS_REQUIRE(reinterpret_cast<uintptr_t>(map) % 16 == 0, "ebos_rectify_map_f64: map must be 16-byte aligned");
  rectify_map_kernel<<<dim3(stream_grid((int64_t)H * W, kBlock)), dim3(kBlock), 0, as_stream(stream)>>>(camera_of(camera), iterations, H, W,
                                                                                                      reinterpret_cast<double2*>(map));
  EBOS_CHECK_LAUNCH("ebos_rectify_map_f64");
  return EBOS_OK;
}

size_t ebos_rectify_scratch_bytes(int64_t n) {
  if (n < 1) n = 1;
  return align256((size_t)n * 4) + align256((size_t)scan_blocks(n) * 4);
}

int ebos_rectify_events_raw(const int16_t* col, const int16_t* row, const void* t, int t_is_int64, const uint8_t* pol, int64_t n,
                            double ticks_per_second, const double* map, int H, int W, int H_out, int W_out, int out_is_f32,
                            void* events_out, int32_t* counts, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(n >= 0 && n <= EBOS_RECTIFY_MAX_EVENTS, "ebos_rectify_events_raw: n = %lld outside 0 .. %lld", (long long)n,
               (long long)EBOS_RECTIFY_MAX_EVENTS);
  EBOS_REQUIRE(H > 0 && W > 0 && H <= 32767 && W <= 32767 && H_out > 0 && W_out > 0, "ebos_rectify_events_raw: bad shape, sensor %d x %d, image %d x %d",
               H, W, H_out, W_out);
  EBOS_REQUIRE(counts && map && ((col && row && t && pol && events_out && scratch) || n == 0), "ebos_rectify_events_raw: NULL buffer");
  EBOS_REQUIRE(ticks_per_second > 0.0 && isfinite(ticks_per_second), "ebos_rectify_events_raw: ticks_per_second must be positive");
  EBOS_REQUIRE(reinterpret_cast<uintptr_t>(map) % 16 == 0 && reinterpret_cast<uintptr_t>(events_out) % 16 == 0,
               "ebos_rectify_events_raw: map and events_out must be 16-byte aligned");
  if (scratch_bytes < ebos_rectify_scratch_bytes(n)) {
    set_error("ebos_rectify_events_raw: scratch too small (%zu < %zu)", scratch_bytes, ebos_rectify_scratch_bytes(n));
    return EBOS_ERR_SCRATCH;
  }
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(counts, 0, 8, s) != hipSuccess) {
    set_error("ebos_rectify_events_raw: hipMemsetAsync failed");
    return EBOS_ERR_LAUNCH;
  }
  if (n == 0) return EBOS_OK;
  RawArgs a = {col, row, t, pol, reinterpret_cast<const double2*>(map), n, ticks_per_second, t_is_int64 ? 1 : 0, H, W, H_out, W_out};
  Scratch sc = carve(scratch, n);
  const dim3 blk(kBlock), g(stream_grid(n, kBlock));
  if (out_is_f32) rectify_flag_kernel<float><<<g, blk, 0, s>>>(a, sc.keep, counts + 1);
  else rectify_flag_kernel<double><<<g, blk, 0, s>>>(a, sc.keep, counts + 1);
  scan_exclusive_i32(sc.keep, n, counts, sc.block_sums, s);
  if (out_is_f32) rectify_scatter_kernel<float><<<g, blk, 0, s>>>(a, sc.keep, static_cast<float*>(events_out));
  else rectify_scatter_kernel<double><<<g, blk, 0, s>>>(a, sc.keep, static_cast<double*>(events_out));
  EBOS_CHECK_LAUNCH("ebos_rectify_events_raw");
  return EBOS_OK;
}

int ebos_undistort_events_f32(const float* events, int64_t n, const double* map_x, const double* map_y, int map_h, int map_w, int h, int w,
                              float* events_out, int32_t* counts, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  return undistort_events<float>(events, n, map_x, map_y, map_h, map_w, h, w, events_out, counts, scratch, scratch_bytes, stream);
}

int ebos_undistort_events_f64(const double* events, int64_t n, const double* map_x, const double* map_y, int map_h, int map_w, int h, int w,
                              double* events_out, int32_t* counts, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  return undistort_events<double>(events, n, map_x, map_y, map_h, map_w, h, w, events_out, counts, scratch, scratch_bytes, stream);
}

int ebos_undistort_image_u8(int B, int Hs, int Ws, const uint8_t* src, int64_t src_sb, int64_t src_sr, const double* camera,
                            const double* M, int H, int W, double border_value, int xmin, int xmax, int ymin, int ymax, uint8_t* out,
                            int64_t out_sb, int64_t out_sr, ebos_stream_t stream) {
  return undistort_image<uint8_t>(B, Hs, Ws, src, src_sb, src_sr, camera, M, H, W, border_value, xmin, xmax, ymin, ymax, out, out_sb, out_sr,
                                  stream);
}

int ebos_undistort_image_f32(int B, int Hs, int Ws, const float* src, int64_t src_sb, int64_t src_sr, const double* camera, const double* M,
                             int H, int W, double border_value, int xmin, int xmax, int ymin, int ymax, float* out, int64_t out_sb,
                             int64_t out_sr, ebos_stream_t stream) {
  return undistort_image<float>(B, Hs, Ws, src, src_sb, src_sr, camera, M, H, W, border_value, xmin, xmax, ymin, ymax, out, out_sb, out_sr,
                                stream);
}

}  // extern "C"
