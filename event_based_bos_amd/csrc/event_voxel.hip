// event_voxel.hip -- the two time-resolved event representations of the reference's utils (src/utils/event_utils.py):
//
//   create_event_voxel (:291-366)                 the DSEC / E2VID voxel grid: every event votes into the eight corners of its cell of
//                                                 a [C, H, W] float64 grid with pol (1 - |xl - x|) (1 - |yl - y|) (1 - |tl - t_norm|),
//                                                 t_norm = (C - 1) (t - t[0]) / (t[-1] - t[0]); optionally normalised by the mean and the
//                                                 unbiased std of its non-zero voxels;
//   generate_discretized_event_volume (:370-440)  the EV-FlowNet / EventGAN volume: positive events in bins [0, T / 2), negative ones in
//                                                 [T / 2, ...), two votes per event, linear in time only, in the events' dtype.
//
// Every product, sum and difference is rounded on its own (fp contract off for the whole file) and in the reference's order, so the
// addends of a voxel are the reference's addends bit for bit; only the order in which they are added is free (float atomics).  A
// tap whose weight is exactly zero is skipped: a sum that starts at +0 is not changed by +-0, and an event on an integer pixel --
// what the loaders emit -- then costs two atomics instead of eight.
//
// ``.int()`` / ``.long()`` of the reference truncate towards zero; a value no int32 holds (NaN, |v| >= 2^31 - 1) has no defined
// result there and votes nowhere here.
//
// The raw-column form takes the window as the grid's outer extent: B windows of a recording issue the launches of one.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace ebos {
namespace {

constexpr int kBlock = 256;
constexpr int kNormPartials = EBOS_VOXEL_NORM_PARTIALS;
static_assert(kNormPartials == kBlock, "the map kernel merges one partial per lane of a workgroup");

__device__ __forceinline__ bool trunc_i32(double v, int* out) {
  if (!(fabs(v) < 2147483647.0)) return false;
  *out = (int)v;
  return true;
}

// the eight votes of one event (src/utils/event_utils.py:333-354), x the width direction
__device__ __forceinline__ void vote8(double x, double y, double pol, double tn, int C, int H, int W, double* __restrict__ out) {
  int x0, y0, t0;
  if (!trunc_i32(x, &x0) || !trunc_i32(y, &y0) || !trunc_i32(tn, &t0)) return;
  const int64_t plane = (int64_t)H * W;
#pragma unroll
  for (int dx = 0; dx < 2; ++dx) {
    const int xl = x0 + dx;
    if (xl < 0 || xl >= W) continue;
    const double wx = pol * (1.0 - fabs((double)xl - x));
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int yl = y0 + dy;
      if (yl < 0 || yl >= H) continue;
      const double wxy = wx * (1.0 - fabs((double)yl - y));
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int tl = t0 + dt;
        if (tl < 0 || tl >= C) continue;
        const double w = wxy * (1.0 - fabs((double)tl - tn));
        if (w != 0.0) atomic_add(out + plane * tl + (int64_t)W * yl + xl, w);
      }
    }
  }
}

__device__ __forceinline__ bool usable_span(double span) { return span != 0.0 && fabs(span) <= 1.79769313486231570e308; }

__global__ __launch_bounds__(kBlock) void voxel_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                       const double* __restrict__ pol, const double* __restrict__ t, int64_t n, int C,
                                                       int H, int W, double* __restrict__ out, int* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const double t_first = t[0];
  const double span = t[n - 1] - t_first;
  const bool ok = usable_span(span);
  if (i == 0) *status = ok ? 1 : 0;
  if (!ok || i >= n) return;
  const double tn = ((double)(C - 1) * (t[i] - t_first)) / span;
  vote8(x[i], y[i], pol[i], tn, C, H, W, out);
}

// ---------------------------------------------------------------------------------------------------- windows of raw columns
struct RawArgs {
  const int16_t* col;
  const int16_t* row;
  const void* t;
  const uint8_t* pol;
  const int64_t* ranges;
  int64_t n_total;
  double ticks_per_second;
  int t_is_64;
  int C, H, W;
  int has_roi, xmin, xmax, ymin, ymax;
  int signed_pol;
  double* out;
  int* valid;
  int64_t* bounds;
};

__device__ __forceinline__ double raw_seconds(const RawArgs& a, int64_t i) {
  const double ticks = a.t_is_64 ? (double)static_cast<const int64_t*>(a.t)[i] : (double)static_cast<const int32_t*>(a.t)[i];
  return ticks / a.ticks_per_second;
}
__device__ __forceinline__ bool raw_keep(const RawArgs& a, int64_t i) {
  if (!a.has_roi) return true;
  const int r = a.row[i], c = a.col[i];
  return r >= a.xmin && r < a.xmax && c >= a.ymin && c < a.ymax;
}
__device__ __forceinline__ void raw_range(const RawArgs& a, int b, int64_t* begin, int64_t* end) {
  int64_t lo = a.ranges[2 * b], hi = a.ranges[2 * b + 1];
  lo = lo < 0 ? 0 : (lo > a.n_total ? a.n_total : lo);
  hi = hi < 0 ? 0 : (hi > a.n_total ? a.n_total : hi);
  *begin = lo;
  *end = hi < lo ? lo : hi;
}

// one workgroup per window: the first and the last event the window keeps (the range ends without a ROI; with one, a scan from
// either end that stops at the first kept event), and whether their times span anything
__global__ __launch_bounds__(kBlock) void raw_bounds_kernel(RawArgs a) {
  __shared__ unsigned long long s_first, s_last;   // index of the first kept event; 1 + index of the last one (0: none)
  const int b = blockIdx.x;
  int64_t begin, end;
  raw_range(a, b, &begin, &end);
  if (threadIdx.x == 0) {
    s_first = ~0ull;
    s_last = 0ull;
  }
  __syncthreads();
  if (!a.has_roi) {
    if (threadIdx.x == 0 && end > begin) {
      s_first = (unsigned long long)begin;
      s_last = (unsigned long long)end;
    }
  } else {
    for (int64_t base = begin; base < end; base += kBlock) {
      const int64_t i = base + threadIdx.x;
      if (i < end && raw_keep(a, i)) atomicMin(&s_first, (unsigned long long)i);
      __syncthreads();
      const bool found = s_first != ~0ull;
      __syncthreads();
      if (found) break;
    }
    for (int64_t top = end; top > begin; top -= kBlock) {
      const int64_t i = top - 1 - threadIdx.x;
      if (i >= begin && raw_keep(a, i)) atomicMax(&s_last, (unsigned long long)(i + 1));
      __syncthreads();
      const bool found = s_last != 0ull;
      __syncthreads();
      if (found) break;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  bool ok = false;
  int64_t first = -1, last = -1;
  if (s_first != ~0ull && s_last != 0ull) {
    first = (int64_t)s_first;
    last = (int64_t)s_last - 1;
    ok = last > first && usable_span(raw_seconds(a, last) - raw_seconds(a, first));
  }
  a.valid[b] = ok ? 1 : 0;
  a.bounds[2 * b] = ok ? first : -1;
  a.bounds[2 * b + 1] = ok ? last : -1;
}

// integer pixels: the weights along x and y are 1 at the pixel and 0 beside it, so two of the eight taps are left, and
// pol * 1 * 1 * wt is pol * wt bit for bit
__global__ __launch_bounds__(kBlock) void raw_voxel_kernel(RawArgs a) {
  const int b = blockIdx.y;
  const int64_t first = a.bounds[2 * b], last = a.bounds[2 * b + 1];
  if (first < 0) return;
  const int64_t i = first + (int64_t)blockIdx.x * kBlock + threadIdx.x;   // (events before `first` and after `last` are dropped ones)
  if (i > last || !raw_keep(a, i)) return;
  const double t_first = raw_seconds(a, first);
  const double span = raw_seconds(a, last) - t_first;
  const double tn = ((double)(a.C - 1) * (raw_seconds(a, i) - t_first)) / span;
  const int xl = (int)a.col[i] - (a.has_roi ? a.ymin : 0), yl = (int)a.row[i] - (a.has_roi ? a.xmin : 0);
  int t0;
  if (xl < 0 || xl >= a.W || yl < 0 || yl >= a.H || !trunc_i32(tn, &t0)) return;
  const double p = a.signed_pol ? (a.pol[i] ? 1.0 : -1.0) : (a.pol[i] ? 1.0 : 0.0);
  double* out = a.out + (int64_t)b * a.C * a.H * a.W + (int64_t)a.W * yl + xl;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const int tl = t0 + dt;
    if (tl < 0 || tl >= a.C) continue;
    const double w = p * (1.0 - fabs((double)tl - tn));
    if (w != 0.0) atomic_add(out + (int64_t)a.H * a.W * tl, w);
  }
}

// ---------------------------------------------------------------------------------------------------- normalisation
// count, mean and sum of squared deviations of the non-zero voxels: Welford per lane, Chan's pairwise merge above it (no
// difference of two large sums, whatever the mean is)
struct Moments {
  double n, mean, m2;
};
__device__ __forceinline__ Moments merge(Moments a, Moments b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Moments r;
  r.n = a.n + b.n;
  const double d = b.mean - a.mean;
  r.mean = a.mean + d * (b.n / r.n);
  r.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / r.n);
  return r;
}
// tree over the workgroup through LDS, in a fixed order; the result is valid in every lane
__device__ __forceinline__ Moments block_merge(Moments m, Moments* red) {
  red[threadIdx.x] = m;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = merge(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  const Moments r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kBlock) void norm_reduce_kernel(const double* __restrict__ grid, int64_t n, Moments* __restrict__ partials) {
  __shared__ Moments red[kBlock];
  const double* g = grid + (int64_t)blockIdx.y * n;
  Moments m = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double v = g[i];
    if (v != 0.0) {
      m.n += 1.0;
      const double d = v - m.mean;
      m.mean += d / m.n;
      m.m2 += d * (v - m.mean);
    }
  }
  m = block_merge(m, red);
  if (threadIdx.x == 0) partials[(int64_t)blockIdx.y * kNormPartials + blockIdx.x] = m;
}

__global__ __launch_bounds__(kBlock) void norm_map_kernel(double* __restrict__ grid, int64_t n, const Moments* __restrict__ partials,
                                                          int n_partials) {
  __shared__ Moments red[kBlock];
  Moments m = {0.0, 0.0, 0.0};
  if ((int)threadIdx.x < n_partials) m = partials[(int64_t)blockIdx.y * kNormPartials + threadIdx.x];
  m = block_merge(m, red);
  if (m.n == 0.0) return;                                     // no voxel is non-zero: the grid stays as it is
  const double std = sqrt(m.m2 / (m.n - 1.0));                // unbiased; NaN for a single voxel, as torch's
  const bool divide = std > 0.0;
  double* g = grid + (int64_t)blockIdx.y * n;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double v = g[i];
    if (v != 0.0) g[i] = divide ? (v - m.mean) / std : v - m.mean;
  }
}

// ---------------------------------------------------------------------------------------------------- discretised event volume
// doubles in the order of their values as unsigned 64-bit keys, for integer atomic min / max (NaN is never offered)
__device__ __forceinline__ unsigned long long order_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ float floor_of(float v) { return floorf(v); }
__device__ __forceinline__ double floor_of(double v) { return floor(v); }
__device__ __forceinline__ float ceil_of(float v) { return ceilf(v); }
__device__ __forceinline__ double ceil_of(double v) { return ceil(v); }

constexpr int kVolumeBounds = EBOS_EVENT_VOLUME_OUT_OF_BOUNDS, kVolumeSpan = EBOS_EVENT_VOLUME_DEGENERATE_SPAN;

// status: [0] flags, [1] key of the smallest time, [2] key of the largest
template <typename T>
__global__ __launch_bounds__(kBlock) void volume_range_kernel(const T* __restrict__ ev, int64_t n, unsigned long long* __restrict__ status) {
  double lo = INFINITY, hi = -INFINITY;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double t = (double)ev[4 * i + 2];
    if (t != t) bad = true;
    lo = fmin(lo, t);
    hi = fmax(hi, t);
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((threadIdx.x & (kWave - 1)) == 0 && lo <= hi) {
    atomicMin(status + 1, order_key(lo));
    atomicMax(status + 2, order_key(hi));
  }
  if (bad) atomicOr(status, (unsigned long long)kVolumeBounds);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void volume_kernel(const T* __restrict__ ev, int64_t n, int nb, int X, int Y, T* __restrict__ out,
                                                        unsigned long long* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const T tmin = (T)key_value(status[1]), tmax = (T)key_value(status[2]);
  const T span = tmax - tmin;
  if (!(span > T(0)) || !((double)span <= 1.79769313486231570e308)) {   // one time only, or none that is a number
    if (i == 0) atomicOr(status, (unsigned long long)kVolumeSpan);
    return;
  }
  if (i >= n) return;
  // ``(nb - 1) / (t_max - t_min)`` on a tensor is torch's __rdiv__: reciprocal() * (nb - 1), two roundings in T
  const T scale = (T(1) / span) * (T)(nb - 1);
  const T xs = ev[4 * i], ys = ev[4 * i + 1], t = ev[4 * i + 2], p = ev[4 * i + 3];
  const T ts = (t - tmin) * scale;
  const T fl = floor_of(ts + (T)1e-8), ce = ceil_of(ts - (T)1e-8);
  const T w_fl = (floor_of(ts) + T(1)) - ts, w_ce = ts - fl;
  bool ok = fabs((double)xs) < 9.0e18 && fabs((double)ys) < 9.0e18;
  const long long x = ok ? (long long)xs : -1, y = ok ? (long long)ys : -1;
  ok = ok && x >= 0 && x < X && y >= 0 && y < Y;
  const int64_t base = (int64_t)X * Y * (p < T(0) ? nb : 0) + (int64_t)Y * x + y;
  const bool ok_fl = ok && fl >= T(0) && fl < (T)nb, ok_ce = ok && ce >= T(0) && ce < (T)nb;
  if (!ok_fl || !ok_ce) atomicOr(status, (unsigned long long)kVolumeBounds);   // the reference's assertions (:397-399)
  if (ok_fl && w_fl != T(0)) atomic_add(out + base + (int64_t)X * Y * (int64_t)fl, w_fl);
  if (ok_ce && w_ce != T(0)) atomic_add(out + base + (int64_t)X * Y * (int64_t)ce, w_ce);
}

template <typename T>
int event_volume(const T* events, int64_t n, int Tn, int X, int Y, T* out, int64_t* status, ebos_stream_t stream, const char* who) {
  EBOS_REQUIRE(events && out && status, "%s: NULL buffer", who);
  EBOS_REQUIRE(n > 0 && n <= 2147483647ll * kBlock, "%s: %lld events", who, (long long)n);
  EBOS_REQUIRE(Tn >= 2 && X > 0 && Y > 0, "%s: bad volume %d x %d x %d (at least two bins)", who, Tn, X, Y);
  const hipStream_t st = as_stream(stream);
  auto* s = reinterpret_cast<unsigned long long*>(status);
  if (hipMemsetAsync(out, 0, sizeof(T) * (size_t)Tn * X * Y, st) != hipSuccess || hipMemsetAsync(s, 0, 32, st) != hipSuccess ||
      hipMemsetAsync(s + 1, 0xff, 8, st) != hipSuccess) {
    set_error("%s: hipMemsetAsync failed", who);
    return EBOS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(volume_range_kernel<T>, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, events, n, s);
  EBOS_CHECK_LAUNCH("ebos_event_volume: volume_range_kernel");
  hipLaunchKernelGGL(volume_kernel<T>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, events, n, Tn / 2, X, Y, out, s);
  EBOS_CHECK_LAUNCH("ebos_event_volume: volume_kernel");
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

using namespace ebos;

extern "C" {

int ebos_event_voxel_f64(const double* x, const double* y, const double* pol, const double* t, int64_t n, int C, int H, int W,
                         double* out, int* status, ebos_stream_t stream) {
  EBOS_REQUIRE(x && y && pol && t && out && status, "ebos_event_voxel_f64: NULL buffer");
  EBOS_REQUIRE(n > 0 && n <= 2147483647ll * kBlock, "ebos_event_voxel_f64: %lld events", (long long)n);
  EBOS_REQUIRE(C > 0 && H > 0 && W > 0, "ebos_event_voxel_f64: bad grid %d x %d x %d", C, H, W);
  const hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(out, 0, sizeof(double) * (size_t)C * H * W, st) != hipSuccess) {
    set_error("ebos_event_voxel_f64: hipMemsetAsync failed");
    return EBOS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(voxel_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, x, y, pol, t, n, C, H, W, out, status);
  EBOS_CHECK_LAUNCH("ebos_event_voxel_f64: voxel_kernel");
  return EBOS_OK;
}

size_t ebos_event_voxel_normalize_scratch_bytes(int B) {
  return B > 0 ? (size_t)B * kNormPartials * sizeof(Moments) : 0;
}

int ebos_event_voxel_normalize_f64(int B, int64_t n, double* grid, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(B > 0 && B <= 65535 && n > 0, "ebos_event_voxel_normalize_f64: %d grids of %lld voxels", B, (long long)n);
  EBOS_REQUIRE(grid && scratch, "ebos_event_voxel_normalize_f64: NULL buffer");
  EBOS_REQUIRE(scratch_bytes >= ebos_event_voxel_normalize_scratch_bytes(B) && reinterpret_cast<uintptr_t>(scratch) % 8 == 0,
               "ebos_event_voxel_normalize_f64: scratch of %zu bytes (need %zu, 8-byte aligned)", scratch_bytes,
               ebos_event_voxel_normalize_scratch_bytes(B));
  const hipStream_t st = as_stream(stream);
  auto* partials = static_cast<Moments*>(scratch);
  const int g = stream_grid(n, kBlock, kNormPartials);
  hipLaunchKernelGGL(norm_reduce_kernel, dim3(g, B), dim3(kBlock), 0, st, grid, n, partials);
  EBOS_CHECK_LAUNCH("ebos_event_voxel_normalize_f64: norm_reduce_kernel");
  hipLaunchKernelGGL(norm_map_kernel, dim3(stream_grid(n, kBlock, 1024), B), dim3(kBlock), 0, st, grid, n, partials, g);
  EBOS_CHECK_LAUNCH("ebos_event_voxel_normalize_f64: norm_map_kernel");
  return EBOS_OK;
}

int ebos_event_volume_f64(const double* events, int64_t n, int T, int X, int Y, double* out, int64_t* status, ebos_stream_t stream) {
  return event_volume<double>(events, n, T, X, Y, out, status, stream, "ebos_event_volume_f64");
}

int ebos_event_volume_f32(const float* events, int64_t n, int T, int X, int Y, float* out, int64_t* status, ebos_stream_t stream) {
  return event_volume<float>(events, n, T, X, Y, out, status, stream, "ebos_event_volume_f32");
}

int ebos_event_voxel_raw_batch(const int16_t* col, const int16_t* row, const void* t, int t_is_64, const uint8_t* pol, int64_t n_total,
                               double ticks_per_second, const int64_t* ranges, int B, int64_t max_len, int C, int H, int W,
                               int has_roi, int xmin, int xmax, int ymin, int ymax, int signed_pol, double* out, int* valid,
                               int64_t* bounds, ebos_stream_t stream) {
  EBOS_REQUIRE(B > 0 && B <= 65535, "ebos_event_voxel_raw_batch: %d windows (1 .. 65535)", B);
  EBOS_REQUIRE(C > 0 && H > 0 && W > 0, "ebos_event_voxel_raw_batch: bad grid %d x %d x %d", C, H, W);
  EBOS_REQUIRE(n_total >= 0 && max_len >= 0 && max_len <= n_total && max_len <= 2147483647ll * kBlock,
               "ebos_event_voxel_raw_batch: %lld events, windows of up to %lld", (long long)n_total, (long long)max_len);
  EBOS_REQUIRE(ranges && out && valid && bounds && (n_total == 0 || (col && row && t && pol)), "ebos_event_voxel_raw_batch: NULL buffer");
  EBOS_REQUIRE(ticks_per_second > 0.0, "ebos_event_voxel_raw_batch: ticks_per_second must be positive");
  EBOS_REQUIRE(!has_roi || (xmax - xmin == H && ymax - ymin == W),
               "ebos_event_voxel_raw_batch: with a ROI the grid is the crop: rows [%d, %d) x columns [%d, %d) is not %d x %d", xmin, xmax,
               ymin, ymax, H, W);
  const hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(out, 0, sizeof(double) * (size_t)B * C * H * W, st) != hipSuccess) {
    set_error("ebos_event_voxel_raw_batch: hipMemsetAsync failed");
    return EBOS_ERR_LAUNCH;
  }
  RawArgs a;
  a.col = col; a.row = row; a.t = t; a.pol = pol; a.ranges = ranges; a.n_total = n_total;
  a.ticks_per_second = ticks_per_second; a.t_is_64 = t_is_64; a.C = C; a.H = H; a.W = W;
  a.has_roi = has_roi; a.xmin = xmin; a.xmax = xmax; a.ymin = ymin; a.ymax = ymax; a.signed_pol = signed_pol;
  a.out = out; a.valid = valid; a.bounds = bounds;
  hipLaunchKernelGGL(raw_bounds_kernel, dim3(B), dim3(kBlock), 0, st, a);
  EBOS_CHECK_LAUNCH("ebos_event_voxel_raw_batch: raw_bounds_kernel");
  if (max_len > 0) {
    hipLaunchKernelGGL(raw_voxel_kernel, dim3((unsigned)((max_len + kBlock - 1) / kBlock), B), dim3(kBlock), 0, st, a);
    EBOS_CHECK_LAUNCH("ebos_event_voxel_raw_batch: raw_voxel_kernel");
  }
  return EBOS_OK;
}

}  // extern "C"
