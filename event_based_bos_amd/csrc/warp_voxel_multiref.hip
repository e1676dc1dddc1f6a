// warp_voxel_multiref.hip -- the time-aware warp scored at K <= EBOS_MULTIREF_MAX reference times for gfx950 / CDNA4: every event is
// displaced by the flow of ITS OWN time bin of a flow voxel [T, 2, H, W] (warp_voxel.hip), once per reference time.  On a plan with
// normalised time another reference time is a scalar shift of every event's dt (iwe_multiref.hip):
//
//   dt_k = dt + s_k (one rounded float32 add; s_k == 0: dt as it is);  x'_k = x - dt_k * V[bin][0][src];  y'_k = y - dt_k * V[bin][1][src]
//
//   forward   iwe_voxel_multiref_tiled_batch_kernel: the tiled forward of warp_voxel.hip (its body, with the shift) over a grid of
//             (tile x split, window, reference): one LDS window per workgroup, the accumulator rule and the spill path unchanged
//   backward  iwe_voxel_multiref_owner_bwd_batch_kernel: the run walk of the pixel-owner backward (owner_bwd_walk) with addends summed
//             over the references -- a
//             lane loads its run's events and gathers their bins' flow ONCE, then sweeps the references over the chunk; no atomics,
//             every cell of d_voxel written, the same bits on every call
// The bin of an event does not depend on the reference; bins are read as min(bins[i], T - 1).
#include <cmath>

#include "tile_configs.h"
#include "warp_voxel_core.h"

namespace ebos {
namespace {

constexpr int kMaxRefs = EBOS_MULTIREF_MAX;
static_assert(kMaxRefs == 4, "Shifts::at selects among four values");

// the shifts travel by value; a reference picks its own with wave-uniform selects (no indexed copy of the argument)
struct Shifts {
  float s0, s1, s2, s3;
  __device__ __forceinline__ float at(int k) const { return k == 0 ? s0 : (k == 1 ? s1 : (k == 2 ? s2 : s3)); }
};

// ---- forward -------------------------------------------------------------------------------------
// blockIdx = (tile x split, window b, reference k): window b reads row b of the offsets and voxel[b], and adds into iwe[b][k]
template <int TH, int TW, int HALO, typename ACC>
__global__ void __launch_bounds__(kTiledBlock)
iwe_voxel_multiref_tiled_batch_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ dts,
                                      const uint8_t* __restrict__ bins, const int32_t* __restrict__ key_offsets,
                                      const float* __restrict__ voxel, int nbins, int H, int W, int tiles_x, int tiles_y, int splits,
                                      int pad_h, int pad_w, Shifts shifts, int K, float* iwe) {
  extern __shared__ double s_raw[];  // [LH][LW] of ACC
  const int64_t b = blockIdx.y;
  const int k = blockIdx.z;
  const int64_t n_keys = (int64_t)tiles_y * tiles_x * (TH * TW);
  iwe_voxel_tiled_body<TH, TW, HALO, ACC, true>(reinterpret_cast<ACC*>(s_raw), xs, ys, dts, nullptr, bins, key_offsets + b * (n_keys + 1),
                                                voxel + b * nbins * 2 * (int64_t)H * W, nbins, H, W, tiles_x, splits, pad_h, pad_w,
                                                iwe + (b * K + k) * (int64_t)(H + 2 * pad_h) * (W + 2 * pad_w), shifts.at(k));
}

// the general kernel with a shift: any event order, global float atomics (the fall-back for an unbuilt (tile, halo))
__global__ void __launch_bounds__(256)
iwe_voxel_shift_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dt,
                       const uint8_t* __restrict__ bins, int64_t n, const float* __restrict__ voxel, int nbins, int H, int W, int pad_h,
                       int pad_w, float shift, float* iwe) {
  iwe_voxel_general_body<true>(x, y, dt, nullptr, bins, n, voxel, nbins, H, W, W, pad_h, pad_w, iwe, shift);
}

template <int TH, int TW, int HALO>
int launch_multiref_tiled_batch(const float* xs, const float* ys, const float* dts, const uint8_t* bins, const int32_t* key_offsets,
                                int B, const float* voxel, int nbins, int H, int W, int splits, int pad_h, int pad_w, Shifts shifts,
                                int K, float* iwe, hipStream_t s) {
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  using ACC = typename TileAcc<TH, TW, HALO>::type;
  constexpr size_t lds = (size_t)LH * LW * sizeof(ACC);
  static_assert(lds <= 160 * 1024, "tile + halo must fit the 160 KiB LDS of a CDNA4 CU");
  const int tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
  auto kern = iwe_voxel_multiref_tiled_batch_kernel<TH, TW, HALO, ACC>;
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess) {
      set_error("ebos_iwe_voxel_multiref_tiled_batch: cannot reserve %zu B of LDS", lds);
      return EBOS_ERR_LAUNCH;
    }
  }
  kern<<<dim3((unsigned)(tiles_y * tiles_x * splits), (unsigned)B, (unsigned)K), dim3(kTiledBlock), lds, s>>>(
      xs, ys, dts, bins, key_offsets, voxel, nbins, H, W, tiles_x, tiles_y, splits, pad_h, pad_w, shifts, K, iwe);
  return EBOS_OK;
}

// ---- backward, pixel-owner form --------------------------------------------------------------------
// the K upstream images of one window: G_k = a_k * g[k] + c_k inside the valid region
struct GradImages {
  const float* g;       // [K, h, w]
  const float* affine;  // [K, 2] or nullptr
  int64_t img;          // h * w
  int h, w, lo;
  __device__ __forceinline__ GradImage at(int k) const {
    GradImage G;
    G.g = g + k * img;
    G.a = affine ? affine[2 * k] : 1.0f;
    G.c = affine ? affine[2 * k + 1] : 0.0f;
    G.h = h;
    G.w = w;
    G.lo = lo;
    return G;
  }
};

__device__ __forceinline__ float shifted(float dt, float s) { return s != 0.0f ? dt + s : dt; }

// one event of source pixel `lin` and bin `kb`: sum over the references of the addend of owner_event_grad (warp_voxel.hip), the
// flow cell gathered once
__device__ __forceinline__ void multiref_event_grad(const GradImages& M, const Shifts& sh, int K, const float* __restrict__ voxel,
                                                    int64_t hw, int64_t lin, int kb, float ex, float ey, float edt, int pad_h, int pad_w,
                                                    float* gx, float* gy) {
  const float* f0 = voxel + (int64_t)kb * 2 * hw;
  const float fu = f0[lin], fv = f0[hw + lin];
  float sx = 0.0f, sy = 0.0f;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const GradImage G = M.at(k);
    const float d = shifted(edt, sh.at(k));
    const Taps f = warped_taps(ex, ey, -d * fu, -d * fv, pad_h, pad_w);
    const float g00 = G.at(f.R, f.C), g10 = G.at(f.R + 1, f.C);
    const float g01 = G.at(f.R, f.C + 1), g11 = G.at(f.R + 1, f.C + 1);
    const float a = 1.0f - f.fr, b = 1.0f - f.fc;
    const float dx = b * (g10 - g00) + f.fc * (g11 - g01);  // dL/dx'_k
    const float dy = a * (g01 - g00) + f.fr * (g11 - g10);  // dL/dy'_k
    sx += -d * dx;
    sy += -d * dy;
  }
  *gx = sx;
  *gy = sy;
}

// events [b0, b0 + cnt) of source pixel `lin`, cnt <= kOwnerChunk: their bins (-1 in the unused slots) and addends (0 there), the
// addend of an event summed over the references in the order k = 0 .. K - 1.  The events and their flow cells are loaded once; the
// reference loop runs over the whole chunk and is not unrolled, so the tap arrays exist once whatever K is.
__device__ __forceinline__ void multiref_owner_chunk(const GradImages& M, const Shifts& sh, int K, const float* __restrict__ x,
                                                     const float* __restrict__ y, const float* __restrict__ dt,
                                                     const uint8_t* __restrict__ bins, const float* __restrict__ voxel, int nbins,
                                                     int64_t hw, int64_t lin, int32_t b0, int cnt, int pad_h, int pad_w,
                                                     int (&kb)[kOwnerChunk], float (&gx)[kOwnerChunk], float (&gy)[kOwnerChunk]) {
  float ex[kOwnerChunk], ey[kOwnerChunk], edt[kOwnerChunk], fu[kOwnerChunk], fv[kOwnerChunk];
#pragma unroll
  for (int j = 0; j < kOwnerChunk; ++j) {
    const bool live = j < cnt;
    const int32_t i = b0 + j;
    kb[j] = live ? clamp_bin(bins[i], nbins) : -1;
    ex[j] = live ? x[i] : 0.0f;
    ey[j] = live ? y[i] : 0.0f;
    edt[j] = live ? dt[i] : 0.0f;
    gx[j] = 0.0f;
    gy[j] = 0.0f;
  }
#pragma unroll
  for (int j = 0; j < kOwnerChunk; ++j) {
    const bool live = j < cnt;
    const float* f0 = voxel + (int64_t)(live ? kb[j] : 0) * 2 * hw;
    fu[j] = live ? f0[lin] : 0.0f;
    fv[j] = live ? f0[hw + lin] : 0.0f;
  }
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const GradImage G = M.at(k);
    const float s = sh.at(k);
    float g00[kOwnerChunk], g10[kOwnerChunk], g01[kOwnerChunk], g11[kOwnerChunk], fr[kOwnerChunk], fc[kOwnerChunk];
#pragma unroll
    for (int j = 0; j < kOwnerChunk; ++j) {
      const bool live = j < cnt;
      const float d = shifted(edt[j], s);
      const Taps f = warped_taps(ex[j], ey[j], -d * fu[j], -d * fv[j], pad_h, pad_w);
      fr[j] = f.fr;
      fc[j] = f.fc;
      g00[j] = live ? G.at(f.R, f.C) : 0.0f;
      g10[j] = live ? G.at(f.R + 1, f.C) : 0.0f;
      g01[j] = live ? G.at(f.R, f.C + 1) : 0.0f;
      g11[j] = live ? G.at(f.R + 1, f.C + 1) : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kOwnerChunk; ++j) {
      const float d = shifted(edt[j], s);
      const float a = 1.0f - fr[j], b = 1.0f - fc[j];
      const float dx = b * (g10[j] - g00[j]) + fc[j] * (g11[j] - g01[j]);  // dL/dx'_k
      const float dy = a * (g01[j] - g00[j]) + fr[j] * (g11[j] - g10[j]);  // dL/dy'_k
      gx[j] += -d * dx;  // (an unused slot: every g = 0)
      gy[j] += -d * dy;
    }
  }
}

// the addends summed over the references, for owner_bwd_walk (warp_voxel_core.h)
struct MultiGrad {
  GradImages M;
  Shifts sh;
  int K;
  const float* __restrict__ x;
  const float* __restrict__ y;
  const float* __restrict__ dt;
  const uint8_t* __restrict__ bins;
  const float* __restrict__ voxel;
  int nbins, pad_h, pad_w;
  int64_t hw;
  __device__ __forceinline__ void chunk(int64_t lin, int32_t b0, int cnt, int (&kb)[kOwnerChunk], float (&gx)[kOwnerChunk],
                                        float (&gy)[kOwnerChunk]) const {
    multiref_owner_chunk(M, sh, K, x, y, dt, bins, voxel, nbins, hw, lin, b0, cnt, pad_h, pad_w, kb, gx, gy);
  }
  __device__ __forceinline__ void event(int64_t lin, int kb, int32_t i, float* gx, float* gy) const {
    multiref_event_grad(M, sh, K, voxel, hw, lin, kb, x[i], y[i], dt[i], pad_h, pad_w, gx, gy);
  }
};

// the key is (pixel key, window = blockIdx.y); window b owns row b of the offsets, voxel[b], g_images[b] [K, h, w], affine[b] [K, 2]
// and d_voxel[b]
__global__ void __launch_bounds__(256)
iwe_voxel_multiref_owner_bwd_batch_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dt,
                                          const uint8_t* __restrict__ bins, const int32_t* __restrict__ key_offsets, WindowBases bases,
                                          const float* __restrict__ voxel, int nbins, int H, int W, int tile_h, int tile_w, int tiles_x,
                                          int64_t n_keys, int pad_h, int pad_w, Shifts shifts, int K,
                                          const float* __restrict__ g_images, const float* __restrict__ affine, int g_lo,
                                          float* d_voxel) {
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nbins * 2 * H * W;
  GradImages M;
  M.h = H + 2 * pad_h;
  M.w = W + 2 * pad_w;
  M.img = (int64_t)M.h * M.w;
  M.g = g_images + (int64_t)b * K * M.img;
  M.affine = affine ? affine + 2 * (int64_t)b * K : nullptr;
  M.lo = g_lo;
  MultiGrad grad;
  grad.M = M, grad.sh = shifts, grad.K = K;
  grad.x = x, grad.y = y, grad.dt = dt, grad.bins = bins, grad.voxel = voxel + b * cells;
  grad.nbins = nbins, grad.pad_h = pad_h, grad.pad_w = pad_w, grad.hw = (int64_t)H * W;
  owner_bwd_walk(grad, bins, key_offsets + (int64_t)b * (n_keys + 1), bases.at[b], bases.at[b + 1], nbins, H, W, tile_h, tile_w, tiles_x,
                 n_keys, d_voxel + b * cells);
}

// K and the shifts of a call, checked; `who` names the entry point
int read_shifts(const char* who, const float* shifts, int K, Shifts* out) {
  EBOS_REQUIRE(K >= 1 && K <= kMaxRefs, "%s: K = %d is outside [1, %d]", who, K, kMaxRefs);
  EBOS_REQUIRE(shifts != nullptr, "%s: shifts is NULL", who);
  float s[kMaxRefs] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < K; ++k) {
    EBOS_REQUIRE(std::isfinite(shifts[k]), "%s: shifts[%d] is not finite", who, k);
    s[k] = shifts[k];
  }
  out->s0 = s[0], out->s1 = s[1], out->s2 = s[2], out->s3 = s[3];
  return EBOS_OK;
}

int multiref_tiled_batch(const char* who, const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                         const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H, int W, int tile_h,
                         int tile_w, int halo, int splits, int pad_h, int pad_w, const float* shifts, int K, float* iwes,
                         ebos_stream_t stream) {
  EBOS_REQUIRE(B >= 1 && B <= kMaxWindows, "%s: B = %d is outside [1, %d]", who, B, kMaxWindows);
  Shifts sh;
  if (int rc = read_shifts(who, shifts, K, &sh)) return rc;
  EBOS_REQUIRE(voxel && iwes && key_offsets && ns, "%s: NULL voxel/iwes/key_offsets/ns", who);
  EBOS_REQUIRE(bins_ok(T), "%s: T = %d is outside [1, 255]", who, T);
  EBOS_REQUIRE(H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && pad_h >= 0 && pad_w >= 0 && splits >= 1 && splits <= 64,
               "%s: bad sizes (splits=%d)", who, splits);
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    EBOS_REQUIRE(ns[b] >= 0, "%s: window %d has n = %lld", who, b, (long long)ns[b]);
    total += ns[b];
    EBOS_REQUIRE(total <= INT32_MAX, "%s: more than INT32_MAX events in the batch", who);
  }
  EBOS_REQUIRE((xs && ys && dts && bins) || total == 0, "%s: NULL event buffer", who);
  if (total == 0) return EBOS_OK;
  hipStream_t s = as_stream(stream);
  const int rc = dispatch_tiled(tile_h, tile_w, halo, [&](auto t) {
    return launch_multiref_tiled_batch<t.th, t.tw, t.halo>(xs, ys, dts, bins, key_offsets, B, voxel, T, H, W, splits, pad_h, pad_w, sh, K, iwes, s);
  });
  if (rc == EBOS_ERR_UNSUPPORTED) {
    // (tile, halo) is no built configuration: the general kernel, window by window and reference by reference
    const int64_t cells = (int64_t)T * 2 * H * W, img = (int64_t)(H + 2 * pad_h) * (W + 2 * pad_w);
    int64_t at = 0;
    for (int b = 0; b < B; ++b) {
      for (int k = 0; k < K && ns[b] > 0; ++k) {
        iwe_voxel_shift_kernel<<<dim3(stream_grid(ns[b], 256)), dim3(256), 0, s>>>(xs + at, ys + at, dts + at, bins + at, ns[b],
                                                                                   voxel + b * cells, T, H, W, pad_h, pad_w, shifts[k],
                                                                                   iwes + ((int64_t)b * K + k) * img);
        EBOS_CHECK_LAUNCH(who);
      }
      at += ns[b];
    }
    return EBOS_OK;
  }
  if (rc != EBOS_OK) return rc;
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

int multiref_owner_bwd_batch(const char* who, const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                             const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H, int W, int tile_h,
                             int tile_w, int pad_h, int pad_w, const float* shifts, int K, const float* g_images, const float* affine,
                             int g_lo, float* d_voxel, ebos_stream_t stream) {
  EBOS_REQUIRE(B >= 1 && B <= kMaxWindows, "%s: B = %d is outside [1, %d]", who, B, kMaxWindows);
  Shifts sh;
  if (int rc = read_shifts(who, shifts, K, &sh)) return rc;
  EBOS_REQUIRE(voxel && g_images && d_voxel, "%s: NULL voxel/g_images/d_voxel", who);
  EBOS_REQUIRE(key_offsets && ns, "%s: key_offsets / ns is NULL (the kernel needs a binned plan)", who);
  EBOS_REQUIRE(bins_ok(T), "%s: T = %d is outside [1, 255]", who, T);
  EBOS_REQUIRE(H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && pad_h >= 0 && pad_w >= 0 && g_lo >= 0, "%s: bad sizes", who);
  WindowBases bases{};
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    EBOS_REQUIRE(ns[b] >= 0, "%s: window %d has n = %lld", who, b, (long long)ns[b]);
    bases.at[b] = (int32_t)total;
    total += ns[b];
    EBOS_REQUIRE(total <= INT32_MAX, "%s: more than INT32_MAX events in the batch", who);
  }
  for (int b = B; b <= kMaxWindows; ++b) bases.at[b] = (int32_t)total;
  EBOS_REQUIRE((xs && ys && dts && bins) || total == 0, "%s: NULL event buffer", who);
  const int tiles_y = (H + tile_h - 1) / tile_h, tiles_x = (W + tile_w - 1) / tile_w;
  const int64_t n_keys = (int64_t)tiles_y * tiles_x * tile_h * tile_w;
  EBOS_REQUIRE(n_keys < INT32_MAX, "%s: %lld keys are more than a plan can hold", who, (long long)n_keys);
  // (an empty window still runs: every cell of its d_voxel is written, with zeros)
  iwe_voxel_multiref_owner_bwd_batch_kernel<<<dim3((unsigned)((n_keys + 255) / 256), (unsigned)B), dim3(256), 0, as_stream(stream)>>>(
      xs, ys, dts, bins, key_offsets, bases, voxel, T, H, W, tile_h, tile_w, tiles_x, n_keys, pad_h, pad_w, sh, K, g_images, affine, g_lo,
      d_voxel);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

int ebos_iwe_voxel_multiref_tiled_batch_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                            const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H,
                                            int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w,
                                            const float* shifts, int K, float* iwes, ebos_stream_t stream) {
  return ebos::multiref_tiled_batch("ebos_iwe_voxel_multiref_tiled_batch", xs, ys, dts, bins, key_offsets, ns, B, voxel, T, H, W, tile_h,
                                    tile_w, halo, splits, pad_h, pad_w, shifts, K, iwes, stream);
}

int ebos_iwe_voxel_multiref_tiled_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                      const int32_t* key_offsets, int64_t n, const float* voxel, int T, int H, int W, int tile_h,
                                      int tile_w, int halo, int splits, int pad_h, int pad_w, const float* shifts, int K, float* iwes,
                                      ebos_stream_t stream) {
  return ebos::multiref_tiled_batch("ebos_iwe_voxel_multiref_tiled", xs, ys, dts, bins, key_offsets, &n, 1, voxel, T, H, W, tile_h,
                                    tile_w, halo, splits, pad_h, pad_w, shifts, K, iwes, stream);
}

int ebos_iwe_voxel_multiref_owner_bwd_batch_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                                const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H,
                                                int W, int tile_h, int tile_w, int pad_h, int pad_w, const float* shifts, int K,
                                                const float* g_images, const float* affine, int g_lo, float* d_voxel,
                                                ebos_stream_t stream) {
  return ebos::multiref_owner_bwd_batch("ebos_iwe_voxel_multiref_owner_bwd_batch", xs, ys, dts, bins, key_offsets, ns, B, voxel, T, H, W,
                                        tile_h, tile_w, pad_h, pad_w, shifts, K, g_images, affine, g_lo, d_voxel, stream);
}

int ebos_iwe_voxel_multiref_owner_bwd_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                          const int32_t* key_offsets, int64_t n, const float* voxel, int T, int H, int W, int tile_h,
                                          int tile_w, int pad_h, int pad_w, const float* shifts, int K, const float* g_images,
                                          const float* affine, int g_lo, float* d_voxel, ebos_stream_t stream) {
  return ebos::multiref_owner_bwd_batch("ebos_iwe_voxel_multiref_owner_bwd", xs, ys, dts, bins, key_offsets, &n, 1, voxel, T, H, W,
                                        tile_h, tile_w, pad_h, pad_w, shifts, K, g_images, affine, g_lo, d_voxel, stream);
}

}  // extern "C"
