// visualize.hip -- the pictures of the reference's visualizer (src/visualizer.py) for B windows per launch: the colour-coded flow
// (``color_optical_flow`` :372-416, with the event-mask forms of ``visualize_optical_flow_on_event_mask`` :271-331 and the shared
// scale of ``visualize_optical_flow_pred_and_gt`` :333-370), the closed event mask (:307-308), the event picture (:459-481), the
// clipped IWE (src/solver/base.py:154-174) and the centred picture of ``standardize_image_center`` (:432-433).
//
// The 8-bit HSV -> RGB step restates OpenCV's ``cv2.cvtColor(hsv, COLOR_HSV2RGB)`` on uint8 (hue 0 - 180): float32 h = H * (6 / 180),
// s = S / 255, v = V / 255, the sector table, * 255 and round half to even -- as tests/_viz_ref.py restates it; it is not checked
// against OpenCV.  Every product and sum is rounded on its own (fp contract off for the whole file), so the float32 sector
// arithmetic agrees with the numpy restatement bit for bit.  The double stage (atan2, sqrt, the divisions) follows numpy's order of
// operations; device atan2 / sqrt / pow may differ from libm in the last bit.
//
// All kernels take the window as the grid's outer extent.  A lane produces four adjacent pixels and stores their bytes as 32-bit
// words where the destination is aligned for it; planes are read as 16-byte pairs of doubles where the source is.  The maximum a
// picture is normalised by is a 64-bit integer atomic max on the bit pattern of the non-negative double: a maximum does not depend
// on the order, so every run gives the same bits.  No floating-point atomics, no scratch.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace ebos {
namespace {

constexpr int kPix = 4;            // adjacent pixels per lane
constexpr int kBlock = 256;
constexpr int kMaxFields = EBOS_VIZ_MAX_FIELDS;

struct FieldTable {
  ebos_viz_field f[kMaxFields];
};

// numpy's ``.astype(np.uint8)`` of a double as x86 computes it for the values met here: truncate towards zero, keep the low byte
// (NaN -> 0).  The pictures only cast non-negative values.
__device__ __forceinline__ uint8_t trunc_u8(double v) {
  if (!(fabs(v) < 9.0e18)) return 0;
  return (uint8_t)(long long)v;
}

__device__ __forceinline__ double finite_or_zero(double v) { return isfinite(v) ? v : 0.0; }

// norm(flow) ** ord as numpy evaluates it: sqrt of the sum of the squares, then sqrt again (ord 0.5), nothing (ord 1) or pow
__device__ __forceinline__ double magnitude(double fx, double fy, int ord_mode, double ord) {
  fx = finite_or_zero(fx);
  fy = finite_or_zero(fy);
  const double n = sqrt(fx * fx + fy * fy);
  return ord_mode == 0 ? sqrt(n) : (ord_mode == 1 ? n : pow(n, ord));
}

__host__ __device__ __forceinline__ int ord_mode_of(double ord) { return ord == 0.5 ? 0 : (ord == 1.0 ? 1 : 2); }

// OpenCV's HSV2RGB on uint8 pixels (hue range 180): modules/imgproc/src/color_hsv, HSV2RGB_b around HSV2RGB_native
__device__ __forceinline__ void hsv2rgb_u8(uint8_t H, uint8_t S, uint8_t V, uint8_t* rgb) {
  float h = (float)H;
  const float s = (float)S * (1.0f / 255.0f);
  const float v = (float)V * (1.0f / 255.0f);
  float r, g, b;
  if (s == 0.0f) {
    r = g = b = v;
  } else {
    h *= 6.0f / 180.0f;
    h = fmodf(h, 6.0f);
    int sector = (int)floorf(h);
    h -= (float)sector;
    if ((unsigned)sector >= 6u) {
      sector = 0;
      h = 0.0f;
    }
    const float t0 = v;
    const float t1 = v * (1.0f - s);
    const float t2 = v * (1.0f - s * h);
    const float t3 = v * (1.0f - s * (1.0f - h));
    // sector_data {b, g, r} = {1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}
    switch (sector) {
      case 0: b = t1; g = t3; r = t0; break;
      case 1: b = t1; g = t0; r = t2; break;
      case 2: b = t3; g = t0; r = t1; break;
      case 3: b = t0; g = t2; r = t1; break;
      case 4: b = t0; g = t1; r = t3; break;
      default: b = t2; g = t1; r = t0; break;
    }
  }
  const float c[3] = {r, g, b};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float q = rintf(c[k] * 255.0f);   // saturate_cast<uchar>(cvRound(.)): half to even, then the clamp
    rgb[k] = (uint8_t)(q < 0.0f ? 0.0f : (q > 255.0f ? 255.0f : q));
  }
}

template <bool VEC>
__device__ __forceinline__ void load4(const double* __restrict__ p, int64_t i, int64_t n, double* v) {
  if (VEC && i + kPix <= n) {
    const double2 a = *reinterpret_cast<const double2*>(p + i), b = *reinterpret_cast<const double2*>(p + i + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k) v[k] = i + k < n ? p[i + k] : 0.0;
  }
}
template <bool VEC>
__device__ __forceinline__ void load4_u8(const uint8_t* __restrict__ p, int64_t i, int64_t n, uint8_t* v) {
  if (VEC && i + kPix <= n) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p + i);
    v[0] = w & 0xff; v[1] = (w >> 8) & 0xff; v[2] = (w >> 16) & 0xff; v[3] = w >> 24;
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k) v[k] = i + k < n ? p[i + k] : 0;
  }
}

// ---------------------------------------------------------------------------------------------------- the scale of a picture
template <bool VEC>
__global__ __launch_bounds__(kBlock) void viz_reduce_kernel(FieldTable tab, int n_fields, int64_t n, int ord_mode, double ord,
                                                            unsigned long long* __restrict__ out) {
  __shared__ double red[kBlock / kWave];
  const int b = blockIdx.z;
  const ebos_viz_field f = tab.f[blockIdx.y];
  const double* x = f.x + (int64_t)b * f.sb;
  const double* y = f.kind == EBOS_VIZ_SCALAR ? nullptr : f.y + (int64_t)b * f.sb;
  const double* x2 = f.kind == EBOS_VIZ_FLOW_PAIR ? f.x2 + (int64_t)b * f.sb2 : nullptr;
  const double* y2 = f.kind == EBOS_VIZ_FLOW_PAIR ? f.y2 + (int64_t)b * f.sb2 : nullptr;
  const uint8_t* mask = f.mask ? f.mask + (int64_t)b * f.mask_sb : nullptr;
  double best = 0.0;
  for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPix; i < n; i += (int64_t)gridDim.x * kBlock * kPix) {
    double vx[kPix], vy[kPix];
    load4<VEC>(x, i, n, vx);
    if (f.kind == EBOS_VIZ_SCALAR) {
#pragma unroll
      for (int k = 0; k < kPix; ++k) best = fmax(best, fabs(vx[k]));   // (fmax: a NaN never wins)
      continue;
    }
    load4<VEC>(y, i, n, vy);
    uint8_t m[kPix] = {1, 1, 1, 1};
    if (mask) load4_u8<VEC>(mask, i, n, m);
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      const double w = m[k] ? 1.0 : 0.0;
      best = fmax(best, magnitude(vx[k] * w, vy[k] * w, ord_mode, ord));
    }
    if (x2) {
      load4<VEC>(x2, i, n, vx);
      load4<VEC>(y2, i, n, vy);
#pragma unroll
      for (int k = 0; k < kPix; ++k) best = fmax(best, magnitude(vx[k], vy[k], ord_mode, ord));
    }
  }
  best = wave_max(best);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) red[wid] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kBlock / kWave; ++k) best = fmax(best, red[k]);
    // best >= 0 and not NaN: the order of doubles is the order of their bit patterns
    if (best > 0.0) atomicMax(out + (int64_t)b * n_fields + blockIdx.y, (unsigned long long)__double_as_longlong(best));
  }
}

// ---------------------------------------------------------------------------------------------------- colour-coded flow
struct RgbArgs {
  const double* x;
  const double* y;
  int64_t sb;
  const double* scale;
  int64_t scale_stride;
  const uint8_t* mask;
  int64_t mask_sb;
  int mask_mode;
  int ord_mode;
  double ord;
  uint8_t* out;
  int64_t n;
};

__device__ __forceinline__ void flow_pixel(double fx, double fy, uint8_t m, double scale, const RgbArgs& a, uint8_t* rgb) {
  if (a.mask && (a.mask_mode & EBOS_VIZ_MASK_MULTIPLY)) {
    const double w = m ? 1.0 : 0.0;
    fx *= w;
    fy *= w;
  }
  const double ang = (atan2(fy, fx) + M_PI) * 180.0 / M_PI / 2.0;
  const double mag = magnitude(fx, fy, a.ord_mode, a.ord);
  const uint8_t H = trunc_u8(ang);
  const uint8_t V = scale > 0.0 ? trunc_u8(255.0 * mag / scale) : 0;   // an all-zero flow is black
  hsv2rgb_u8(H, 255, V, rgb);
  if (a.mask && !m) {
    if (a.mask_mode & EBOS_VIZ_MASK_BLACK) rgb[0] = rgb[1] = rgb[2] = 0;
    if (a.mask_mode & EBOS_VIZ_MASK_WHITE) rgb[0] = rgb[1] = rgb[2] = 255;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void viz_flow_rgb_kernel(RgbArgs a) {
  const int b = blockIdx.y;
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPix;
  if (i >= a.n) return;
  const double scale = a.scale[(int64_t)b * a.scale_stride];
  double vx[kPix], vy[kPix];
  uint8_t m[kPix] = {1, 1, 1, 1};
  load4<VEC>(a.x + (int64_t)b * a.sb, i, a.n, vx);
  load4<VEC>(a.y + (int64_t)b * a.sb, i, a.n, vy);
  if (a.mask) load4_u8<VEC>(a.mask + (int64_t)b * a.mask_sb, i, a.n, m);
  uint8_t px[kPix * 3];
#pragma unroll
  for (int k = 0; k < kPix; ++k) flow_pixel(vx[k], vy[k], m[k], scale, a, px + 3 * k);
  uint8_t* out = a.out + ((int64_t)b * a.n + i) * 3;
  if (VEC && i + kPix <= a.n) {   // 12 bytes at a multiple of 12 from a 4-byte aligned base
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
#pragma unroll
    for (int w = 0; w < 3; ++w)
      o[w] = (uint32_t)px[4 * w] | ((uint32_t)px[4 * w + 1] << 8) | ((uint32_t)px[4 * w + 2] << 16) | ((uint32_t)px[4 * w + 3] << 24);
  } else {
    for (int k = 0; k < kPix && i + k < a.n; ++k) {
      out[3 * k] = px[3 * k];
      out[3 * k + 1] = px[3 * k + 1];
      out[3 * k + 2] = px[3 * k + 2];
    }
  }
}

__global__ __launch_bounds__(kBlock) void viz_hsv2rgb_kernel(const uint8_t* __restrict__ hsv, uint8_t* __restrict__ rgb, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint8_t c[3];
  hsv2rgb_u8(hsv[3 * i], hsv[3 * i + 1], hsv[3 * i + 2], c);
  rgb[3 * i] = c[0];
  rgb[3 * i + 1] = c[1];
  rgb[3 * i + 2] = c[2];
}

// ---------------------------------------------------------------------------------------------------- the closed event mask
constexpr int kTileW = 64, kTileH = 16;   // outputs per workgroup: 256 lanes x four adjacent pixels

template <bool VEC>
__global__ __launch_bounds__(kBlock) void viz_mask_close_kernel(const uint8_t* __restrict__ mask, int64_t mask_sb, int H, int W,
                                                                uint8_t* __restrict__ out) {
  // src: the tile with a 2-pixel halo (0 outside the image: never wins the dilation); dil: the dilated tile with a 1-pixel halo
  // (1 outside the image: never loses the erosion)
  __shared__ uint8_t src[kTileH + 4][kTileW + 4];
  __shared__ uint8_t dil[kTileH + 2][kTileW + 2];
  const int b = blockIdx.z;
  const int r0 = blockIdx.y * kTileH, c0 = blockIdx.x * kTileW;
  const uint8_t* in = mask + (int64_t)b * mask_sb;
  for (int t = threadIdx.x; t < (kTileH + 4) * (kTileW + 4); t += kBlock) {
    const int lr = t / (kTileW + 4), lc = t % (kTileW + 4);
    const int r = r0 + lr - 2, c = c0 + lc - 2;
    src[lr][lc] = (r >= 0 && r < H && c >= 0 && c < W) ? (in[(int64_t)r * W + c] != 0) : 0;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < (kTileH + 2) * (kTileW + 2); t += kBlock) {
    const int lr = t / (kTileW + 2), lc = t % (kTileW + 2);
    const int r = r0 + lr - 1, c = c0 + lc - 1;
    const int sr = lr + 1, sc = lc + 1;
    const uint8_t d = src[sr][sc] | src[sr - 1][sc] | src[sr + 1][sc] | src[sr][sc - 1] | src[sr][sc + 1];
    dil[lr][lc] = (r >= 0 && r < H && c >= 0 && c < W) ? d : 1;
  }
  __syncthreads();
  const int lr = threadIdx.x / (kTileW / kPix), lc = (threadIdx.x % (kTileW / kPix)) * kPix;
  const int r = r0 + lr, c = c0 + lc;
  if (r >= H || c >= W) return;
  uint8_t v[kPix];
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    const int dr = lr + 1, dc = lc + k + 1;
    v[k] = dil[dr][dc] & dil[dr - 1][dc] & dil[dr + 1][dc] & dil[dr][dc - 1] & dil[dr][dc + 1];
  }
  uint8_t* o = out + ((int64_t)b * H + r) * W + c;
  if (VEC && c + kPix <= W) {
    *reinterpret_cast<uint32_t*>(o) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  } else {
    for (int k = 0; k < kPix && c + k < W; ++k) o[k] = v[k];
  }
}

// ---------------------------------------------------------------------------------------------------- grey pictures
struct GrayArgs {
  int mode;
  int H, W, pad;           // source planes are H x W; the picture is their inside, (H - 2 pad) x (W - 2 pad)
  const double* a;
  int64_t a_sb;
  const double* b;
  int64_t b_sb;
  double max_scale;
  const double* scale;
  int64_t scale_stride;
  uint8_t* out;
};

template <bool VEC_IN, bool VEC_OUT>
__global__ __launch_bounds__(kBlock) void viz_gray_kernel(GrayArgs g) {
  const int w = blockIdx.z;
  const int Ho = g.H - 2 * g.pad, Wo = g.W - 2 * g.pad;
  const int col = (blockIdx.x * kWave + (threadIdx.x & (kWave - 1))) * kPix;
  const int row = blockIdx.y * (kBlock / kWave) + threadIdx.x / kWave;
  if (row >= Ho || col >= Wo) return;
  const int64_t at = (int64_t)(row + g.pad) * g.W + g.pad + col;   // first source element of this lane
  const int64_t end = at + (Wo - col);                             // one past the last picture column of this row
  double va[kPix], vb[kPix] = {0.0, 0.0, 0.0, 0.0};
  load4<VEC_IN>(g.a + (int64_t)w * g.a_sb, at, end, va);
  if (g.b) load4<VEC_IN>(g.b + (int64_t)w * g.b_sb, at, end, vb);
  const double scale = g.scale ? g.scale[(int64_t)w * g.scale_stride] : 0.0;
  uint8_t v[kPix];
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    if (g.mode == EBOS_VIZ_GRAY_EVENT) {            // clip(20 (n+ - n-) + background, 0, 255)
      const double t = (va[k] - vb[k]) * 20.0 + g.max_scale;
      v[k] = trunc_u8(fmin(fmax(t, 0.0), 255.0));
    } else if (g.mode == EBOS_VIZ_GRAY_IWE) {       // 255 - uint8(clip(max_scale iwe, 0, 255))
      const double t = g.max_scale * (va[k] + vb[k]);
      v[k] = (uint8_t)(255 - trunc_u8(fmin(fmax(t, 0.0), 255.0)));
    } else {                                        // uint8(a / max|a| * 127 + 128); an all-zero field is 128
      v[k] = scale > 0.0 ? trunc_u8(va[k] / scale * 127.0 + 128.0) : 128;
    }
  }
  uint8_t* o = g.out + ((int64_t)w * Ho + row) * Wo + col;
  if (VEC_OUT && col + kPix <= Wo) {
    *reinterpret_cast<uint32_t*>(o) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  } else {
    for (int k = 0; k < kPix && col + k < Wo; ++k) o[k] = v[k];
  }
}

bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
bool plane_ok(const double* p, int64_t sb) { return !p || (aligned(p, 16) && sb % 2 == 0); }
bool bytes_ok(const uint8_t* p, int64_t sb) { return !p || (aligned(p, 4) && sb % 4 == 0); }

}  // namespace
}  // namespace ebos

using namespace ebos;

extern "C" {

int ebos_viz_reduce_f64(int B, int H, int W, const ebos_viz_field* fields, int n_fields, double ord, double* out,
                        ebos_stream_t stream) {
  EBOS_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "ebos_viz_reduce_f64: bad shape B = %d, %d x %d", B, H, W);
  EBOS_REQUIRE(fields && n_fields > 0 && n_fields <= kMaxFields, "ebos_viz_reduce_f64: %d fields (1 .. %d)", n_fields, kMaxFields);
  EBOS_REQUIRE(out, "ebos_viz_reduce_f64: out is NULL");
  EBOS_REQUIRE(ord == ord, "ebos_viz_reduce_f64: ord is NaN");
  const int64_t n = (int64_t)H * W;
  FieldTable tab = {};
  bool vec = true;
  for (int k = 0; k < n_fields; ++k) {
    const ebos_viz_field& f = fields[k];
    EBOS_REQUIRE(f.kind == EBOS_VIZ_FLOW || f.kind == EBOS_VIZ_FLOW_PAIR || f.kind == EBOS_VIZ_SCALAR,
                 "ebos_viz_reduce_f64: field %d has kind %d", k, f.kind);
    EBOS_REQUIRE(f.x && (f.kind == EBOS_VIZ_SCALAR || f.y), "ebos_viz_reduce_f64: field %d has a NULL plane", k);
    EBOS_REQUIRE(f.kind != EBOS_VIZ_FLOW_PAIR || (f.x2 && f.y2), "ebos_viz_reduce_f64: pair field %d lacks its second flow", k);
    EBOS_REQUIRE((B == 1 || f.sb >= n) && (B == 1 || f.kind != EBOS_VIZ_FLOW_PAIR || f.sb2 >= n) &&
                     (B == 1 || !f.mask || f.mask_sb >= n),
                 "ebos_viz_reduce_f64: field %d: a window stride is below H W", k);
    vec = vec && plane_ok(f.x, f.sb) && plane_ok(f.kind == EBOS_VIZ_SCALAR ? nullptr : f.y, f.sb) &&
          (f.kind != EBOS_VIZ_FLOW_PAIR || (plane_ok(f.x2, f.sb2) && plane_ok(f.y2, f.sb2))) && bytes_ok(f.mask, f.mask_sb);
    tab.f[k] = f;
  }
  const hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(out, 0, sizeof(double) * (size_t)B * n_fields, st) != hipSuccess) {
    set_error("ebos_viz_reduce_f64: hipMemsetAsync failed");
    return EBOS_ERR_LAUNCH;
  }
  // enough workgroups per (window, field) to fill the card at B = 1, no more than the plane has work for
  const dim3 grid(stream_grid((n + kPix - 1) / kPix, kBlock, 256), n_fields, B);
  auto* bits = reinterpret_cast<unsigned long long*>(out);
  if (vec)
    hipLaunchKernelGGL(viz_reduce_kernel<true>, grid, dim3(kBlock), 0, st, tab, n_fields, n, ord_mode_of(ord), ord, bits);
  else
    hipLaunchKernelGGL(viz_reduce_kernel<false>, grid, dim3(kBlock), 0, st, tab, n_fields, n, ord_mode_of(ord), ord, bits);
  EBOS_CHECK_LAUNCH("ebos_viz_reduce_f64: viz_reduce_kernel");
  return EBOS_OK;
}

int ebos_viz_flow_rgb_u8(int B, int H, int W, const double* x, const double* y, int64_t sb, const double* scale,
                         int64_t scale_stride, const uint8_t* mask, int64_t mask_sb, int mask_mode, double ord, uint8_t* out,
                         ebos_stream_t stream) {
  EBOS_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "ebos_viz_flow_rgb_u8: bad shape B = %d, %d x %d", B, H, W);
  EBOS_REQUIRE(x && y && scale && out, "ebos_viz_flow_rgb_u8: NULL buffer");
  const int64_t n = (int64_t)H * W;
  EBOS_REQUIRE(B == 1 || (sb >= n && scale_stride >= 0 && (!mask || mask_sb >= n)), "ebos_viz_flow_rgb_u8: a window stride is below H W");
  EBOS_REQUIRE((mask_mode & ~(EBOS_VIZ_MASK_MULTIPLY | EBOS_VIZ_MASK_BLACK | EBOS_VIZ_MASK_WHITE)) == 0 &&
                   (mask_mode & (EBOS_VIZ_MASK_BLACK | EBOS_VIZ_MASK_WHITE)) != (EBOS_VIZ_MASK_BLACK | EBOS_VIZ_MASK_WHITE),
               "ebos_viz_flow_rgb_u8: mask_mode %d", mask_mode);
  EBOS_REQUIRE(ord == ord, "ebos_viz_flow_rgb_u8: ord is NaN");
  RgbArgs a;
  a.x = x; a.y = y; a.sb = sb; a.scale = scale; a.scale_stride = scale_stride;
  a.mask = mask; a.mask_sb = mask_sb; a.mask_mode = mask_mode;
  a.ord_mode = ord_mode_of(ord); a.ord = ord; a.out = out; a.n = n;
  const bool vec = plane_ok(x, sb) && plane_ok(y, sb) && bytes_ok(mask, mask_sb) && aligned(out, 4) && (n * 3) % 4 == 0;
  const int64_t groups = (n + (int64_t)kBlock * kPix - 1) / ((int64_t)kBlock * kPix);
  EBOS_REQUIRE(groups <= 2147483647ll, "ebos_viz_flow_rgb_u8: %d x %d is too large", H, W);
  const dim3 grid((unsigned)groups, B);
  if (vec)
    hipLaunchKernelGGL(viz_flow_rgb_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(viz_flow_rgb_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), a);
  EBOS_CHECK_LAUNCH("ebos_viz_flow_rgb_u8: viz_flow_rgb_kernel");
  return EBOS_OK;
}

int ebos_viz_hsv2rgb_u8(int64_t n, const uint8_t* hsv, uint8_t* rgb, ebos_stream_t stream) {
  EBOS_REQUIRE(n > 0 && n <= 2147483647ll * kBlock, "ebos_viz_hsv2rgb_u8: %lld pixels", (long long)n);
  EBOS_REQUIRE(hsv && rgb, "ebos_viz_hsv2rgb_u8: NULL buffer");
  hipLaunchKernelGGL(viz_hsv2rgb_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), hsv, rgb, n);
  EBOS_CHECK_LAUNCH("ebos_viz_hsv2rgb_u8: viz_hsv2rgb_kernel");
  return EBOS_OK;
}

int ebos_viz_mask_close_u8(int B, int H, int W, const uint8_t* mask, int64_t mask_sb, uint8_t* out, ebos_stream_t stream) {
  EBOS_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "ebos_viz_mask_close_u8: bad shape B = %d, %d x %d", B, H, W);
  EBOS_REQUIRE(mask && out && mask != out, "ebos_viz_mask_close_u8: NULL or aliased buffer");
  EBOS_REQUIRE(B == 1 || mask_sb >= (int64_t)H * W, "ebos_viz_mask_close_u8: window stride %lld is below H W", (long long)mask_sb);
  const int gy = (H + kTileH - 1) / kTileH;
  EBOS_REQUIRE(gy <= 65535, "ebos_viz_mask_close_u8: %d rows are too many", H);
  const dim3 grid((W + kTileW - 1) / kTileW, gy, B);
  if (aligned(out, 4) && W % 4 == 0)
    hipLaunchKernelGGL(viz_mask_close_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), mask, mask_sb, H, W, out);
  else
    hipLaunchKernelGGL(viz_mask_close_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), mask, mask_sb, H, W, out);
  EBOS_CHECK_LAUNCH("ebos_viz_mask_close_u8: viz_mask_close_kernel");
  return EBOS_OK;
}

int ebos_viz_gray_u8(int mode, int B, int H, int W, int pad, const double* a, int64_t a_sb, const double* b, int64_t b_sb,
                     double max_scale, const double* scale, int64_t scale_stride, uint8_t* out, ebos_stream_t stream) {
  EBOS_REQUIRE(mode == EBOS_VIZ_GRAY_EVENT || mode == EBOS_VIZ_GRAY_IWE || mode == EBOS_VIZ_GRAY_CENTER, "ebos_viz_gray_u8: mode %d", mode);
  EBOS_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && pad >= 0 && 2 * pad < H && 2 * pad < W,
               "ebos_viz_gray_u8: bad shape B = %d, %d x %d, padding %d", B, H, W, pad);
  EBOS_REQUIRE(a && out, "ebos_viz_gray_u8: NULL buffer");
  EBOS_REQUIRE(mode != EBOS_VIZ_GRAY_EVENT || b, "ebos_viz_gray_u8: the event picture needs the negative counts");
  EBOS_REQUIRE(mode != EBOS_VIZ_GRAY_CENTER || (scale && !b), "ebos_viz_gray_u8: the centred picture takes one plane and its scale");
  EBOS_REQUIRE(max_scale == max_scale, "ebos_viz_gray_u8: max_scale is NaN");
  const int64_t n = (int64_t)H * W;
  EBOS_REQUIRE(B == 1 || (a_sb >= n && (!b || b_sb >= n)), "ebos_viz_gray_u8: a window stride is below H W");
  const int Ho = H - 2 * pad, Wo = W - 2 * pad;
  const int gy = (Ho + kBlock / kWave - 1) / (kBlock / kWave);
  EBOS_REQUIRE(gy <= 65535, "ebos_viz_gray_u8: %d rows are too many", Ho);
  GrayArgs g;
  g.mode = mode; g.H = H; g.W = W; g.pad = pad; g.a = a; g.a_sb = a_sb; g.b = b; g.b_sb = b_sb;
  g.max_scale = max_scale; g.scale = scale; g.scale_stride = scale_stride; g.out = out;
  // a lane's first source element is (row + pad) W + pad + 4 j: even when W and pad are
  const bool vin = plane_ok(a, a_sb) && plane_ok(b, b_sb) && W % 2 == 0 && pad % 2 == 0;
  const bool vout = aligned(out, 4) && Wo % 4 == 0;
  const dim3 grid((Wo + kWave * kPix - 1) / (kWave * kPix), gy, B);
  const hipStream_t st = as_stream(stream);
  if (vin && vout)
    hipLaunchKernelGGL((viz_gray_kernel<true, true>), grid, dim3(kBlock), 0, st, g);
  else if (vin)
    hipLaunchKernelGGL((viz_gray_kernel<true, false>), grid, dim3(kBlock), 0, st, g);
  else if (vout)
    hipLaunchKernelGGL((viz_gray_kernel<false, true>), grid, dim3(kBlock), 0, st, g);
  else
    hipLaunchKernelGGL((viz_gray_kernel<false, false>), grid, dim3(kBlock), 0, st, g);
  EBOS_CHECK_LAUNCH("ebos_viz_gray_u8: viz_gray_kernel");
  return EBOS_OK;
}

}  // extern "C"
