// iwe_multiref.hip -- the multi-reference focus objective for gfx950 / CDNA4: the IWEs of ONE dense flow at K <= 4 reference times
// from one pass over a binned plan, and their backward summed by the owner of each source pixel's run.
//
// A plan built with normalised time and reference fraction f holds dt = (t - tmin) / (tmax - tmin) - f.  The dt of reference
// fraction r is dt + (f - r): a per-reference scalar shift (shifts[k], float32, from the host).  So an event is decoded once, its
// flow cell gathered once, and the K warped positions differ in one addition:
//
//   warp     dt_k = dt + shifts[k];  x'_k = x - dt_k * flow[0][pix];  y'_k = y - dt_k * flow[1][pix];  pix at (trunc x, trunc y)
//   forward  iwe_multiref_tiled_kernel: iwe_dense_tiled_kernel of iwe_fused.hip with K LDS windows of tile + halo per workgroup
//            (votes, eps and the spill path beyond the halo are that kernel's); f64 windows where K of them fit the LDS, else f32
//   owner    iwe_multiref_owner_bwd_kernel: iwe_voxel_owner_bwd_kernel of warp_voxel.hip with the sum over references inside the
//            walk of a run -- all events of a source pixel share ONE flow cell, so its owner writes d_flow once: no atomics, every
//            cell written, the same bits on every call
#include <cmath>

#include "tile_configs.h"
#include "warp_footprint.h"

namespace ebos {
namespace {

constexpr int kMaxRef = EBOS_MULTIREF_MAX;
constexpr size_t kLdsBytes = 160 * 1024;

struct Shifts {
  float at[kMaxRef];
};

// ---- tiled forward: K LDS-privatised windows per workgroup ---------------------------------------
constexpr int kTiledBlock = 1024;

template <int TH, int TW, int HALO, typename ACC>
__global__ void __launch_bounds__(kTiledBlock)
iwe_multiref_tiled_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ dts,
                          const int32_t* __restrict__ key_offsets, int32_t n, const float* __restrict__ flow, int H, int W,
                          int tiles_x, int splits, int pad_h, int pad_w, Shifts shifts, int K, float* iwes) {
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  extern __shared__ double s_raw[];  // [K][LH][LW] of ACC
  ACC* s_img = reinterpret_cast<ACC*>(s_raw);

  const int tile = blockIdx.x / splits, part = blockIdx.x - tile * splits;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  // (a run never leaves the plan's events, whatever the table holds)
  const int32_t beg = min(max(key_offsets[tile * (TH * TW)], 0), n);
  const int32_t end = min(max(key_offsets[(tile + 1) * (TH * TW)], beg), n);
  if (beg == end) return;
  int32_t chunk = (end - beg + splits - 1) / splits;
  chunk = (chunk + kWave - 1) & ~(kWave - 1);
  const int32_t my_beg = beg + part * chunk;
  const int32_t my_end = min(end, my_beg + chunk);
  if (my_beg >= my_end) return;

  for (int i = threadIdx.x; i < K * LH * LW; i += kTiledBlock) s_img[i] = ACC(0);
  __syncthreads();

  const int64_t hw = (int64_t)H * W;
  const int h = H + 2 * pad_h, w = W + 2 * pad_w;
  const int64_t img = (int64_t)h * w;
  // LDS cell (0,0) <-> un-padded image pixel (oy, ox); padded pixel (oy + pad_h, ox + pad_w)
  const int oy = ty * TH - HALO, ox = tx * TW - HALO;

  // kUnroll events in flight per thread: the coalesced SoA loads first, then ONE flow gather per event, then K sets of LDS atomics
  constexpr int kUnroll = 4;
  for (int32_t base = my_beg + threadIdx.x; base < my_end; base += kTiledBlock * kUnroll) {
    float ex[kUnroll], ey[kUnroll], edt[kUnroll], fu[kUnroll], fv[kUnroll];
    bool live[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const int32_t i = base + j * kTiledBlock;
      live[j] = i < my_end;
      ex[j] = live[j] ? xs[i] : -1.0f;  // -1 marks a dead slot
      ey[j] = live[j] ? ys[i] : 0.0f;
      edt[j] = live[j] ? dts[i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const bool finite = ex[j] > -1e9f && ex[j] < 1e9f && ey[j] > -1e9f && ey[j] < 1e9f;
      const int64_t lin = finite ? (int64_t)(int)ex[j] * W + (int)ey[j] : -1;  // binned events have a valid source pixel
      live[j] = live[j] && lin >= 0 && lin < hw;
      fu[j] = live[j] ? flow[lin] : 0.0f;
      fv[j] = live[j] ? flow[hw + lin] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      if (!live[j]) continue;
#pragma unroll
      for (int k = 0; k < kMaxRef; ++k) {
        if (k >= K) break;
        const float dtk = edt[j] + shifts.at[k];
        const Taps f = warped_taps(ex[j], ey[j], -dtk * fu[j], -dtk * fv[j], 0, 0);  // un-padded coordinates
        const float fr = f.fr, fc = f.fc;
        const float a = 1.0f - fr, b = 1.0f - fc;
        const float w00 = a * b, w10 = fr * b, w01 = a * fc, w11 = fr * fc;
        const int rl = f.R - oy, cl = f.C - ox;  // LDS cell of the top-left tap
        if (f.ok && rl >= 0 && rl < LH - 1 && cl >= 0 && cl < LW - 1) {
          ACC* p = &s_img[k * (LH * LW) + rl * LW + cl];
          atomic_add(p, (ACC)w00);
          atomic_add(p + LW, (ACC)w10);
          atomic_add(p + 1, (ACC)w01);
          atomic_add(p + LW + 1, (ACC)w11);
        } else if (f.ok) {
          // beyond the halo: straight to the image, so any displacement stays exact
          float* iwe = iwes + k * img;
          const int R = f.R + pad_h, C = f.C + pad_w;
          const bool rr0 = R >= 0 && R < h, rr1 = R + 1 >= 0 && R + 1 < h;
          const bool cc0 = C >= 0 && C < w, cc1 = C + 1 >= 0 && C + 1 < w;
          const int64_t gb = (int64_t)R * w + C;
          if (rr0 && cc0) atomic_add(&iwe[gb], w00);
          if (rr1 && cc0) atomic_add(&iwe[gb + w], w10);
          if (rr0 && cc1) atomic_add(&iwe[gb + 1], w01);
          if (rr1 && cc1) atomic_add(&iwe[gb + w + 1], w11);
        }
      }
    }
  }
  __syncthreads();

  // flush: consecutive lanes -> consecutive columns of one image row, window after window
  const int gy0 = oy + pad_h, gx0 = ox + pad_w;
  for (int k = 0; k < K; ++k) {
    float* iwe = iwes + k * img;
    const ACC* win = s_img + k * (LH * LW);
    for (int i = threadIdx.x; i < LH * LW; i += kTiledBlock) {
      const float v = (float)win[i];
      if (v == 0.0f) continue;
      const int rl = i / LW, cl = i - rl * LW;
      const int R = gy0 + rl, C = gx0 + cl;
      if (R >= 0 && R < h && C >= 0 && C < w) atomic_add(&iwe[(int64_t)R * w + C], v);
    }
  }
}

// TileAcc's rule applied to K windows: 2 = f64 where the K windows fit the LDS, 1 = f32, 0 = they do not fit
int fits_cells(size_t cells, int K) {
  if (K < 1 || K > kMaxRef) return 0;
  if (cells * K * sizeof(double) <= kLdsBytes) return 2;
  if (cells * K * sizeof(float) <= kLdsBytes) return 1;
  return 0;
}

template <int TH, int TW, int HALO, typename ACC>
int launch_multiref_acc(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int32_t n, const float* flow,
                        int H, int W, int splits, int pad_h, int pad_w, const Shifts& shifts, int K, float* iwes, hipStream_t s) {
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  const size_t lds = (size_t)K * LH * LW * sizeof(ACC);
  if (lds > kLdsBytes) {
    set_error("ebos_iwe_dense_multiref_tiled: %d windows of tile %dx%d halo %d do not fit the LDS", K, TH, TW, HALO);
    return EBOS_ERR_UNSUPPORTED;
  }
  const int tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
  auto kern = iwe_multiref_tiled_kernel<TH, TW, HALO, ACC>;
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess) {
      set_error("ebos_iwe_dense_multiref_tiled: cannot reserve %zu B of LDS", lds);
      return EBOS_ERR_LAUNCH;
    }
  }
  kern<<<dim3((unsigned)(tiles_y * tiles_x * splits)), dim3(kTiledBlock), lds, s>>>(xs, ys, dts, key_offsets, n, flow, H, W, tiles_x,
                                                                                     splits, pad_h, pad_w, shifts, K, iwes);
  return EBOS_OK;
}

template <int TH, int TW, int HALO>
int launch_multiref(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int32_t n, const float* flow, int H,
                    int W, int splits, int pad_h, int pad_w, const Shifts& shifts, int K, float* iwes, hipStream_t s) {
  constexpr size_t cells = (size_t)(TH + 2 * HALO) * (TW + 2 * HALO);
  if constexpr (cells * sizeof(double) <= kLdsBytes) {  // (a configuration whose single window is f32 has no f64 kernel)
    if (fits_cells(cells, K) == 2)
      return launch_multiref_acc<TH, TW, HALO, double>(xs, ys, dts, key_offsets, n, flow, H, W, splits, pad_h, pad_w, shifts, K, iwes, s);
  }
  return launch_multiref_acc<TH, TW, HALO, float>(xs, ys, dts, key_offsets, n, flow, H, W, splits, pad_h, pad_w, shifts, K, iwes, s);
}

// ---- backward, pixel-owner form ------------------------------------------------------------------
// One lane per key walks its source pixel's run and is the only writer of that pixel's two cells of d_flow.
//   run <= kOwnerHot     kOwnerChunk events at a time: the events, then per reference the taps of the chunk's events in flight together,
//                        added event by event; the order is (chunk, reference, event) -- fixed by the plan
//   longer (a hot pixel) the whole wave walks the run 64 events at a time; each lane sums its event over the references, a butterfly
//                        sums the lanes (a fixed tree, the same total in every lane), added to the running sum
constexpr int kOwnerChunk = 4;
constexpr int kOwnerHot = 64;

struct GradImages {
  const float* g;  // [K, h, w]
  float a[kMaxRef], c[kMaxRef];  // G_k = a_k * g[k] + c_k inside the valid region
  int h, w, lo;
  int64_t img;
  __device__ __forceinline__ float at(int k, int R, int C) const {
    if (R < lo || R >= h - lo || C < lo || C >= w - lo) return 0.0f;
    return a[k] * g[k * img + (int64_t)R * w + C] + c[k];
  }
};

// sum over the references of -dt_k * dL/d(x'_k, y'_k) for one event whose flow cell holds (u, v)
__device__ __forceinline__ void owner_event_grad(const GradImages& G, const Shifts& shifts, int K, float ex, float ey, float edt, float u,
                                                 float v, int pad_h, int pad_w, float* gx, float* gy) {
  float sx = 0.0f, sy = 0.0f;
#pragma unroll
  for (int k = 0; k < kMaxRef; ++k) {
    if (k >= K) break;
    const float dtk = edt + shifts.at[k];
    const Taps f = warped_taps(ex, ey, -dtk * u, -dtk * v, pad_h, pad_w);
    const float g00 = G.at(k, f.R, f.C), g10 = G.at(k, f.R + 1, f.C);
    const float g01 = G.at(k, f.R, f.C + 1), g11 = G.at(k, f.R + 1, f.C + 1);
    const float a = 1.0f - f.fr, b = 1.0f - f.fc;
    const float dx = b * (g10 - g00) + f.fc * (g11 - g01);  // dL/dx'_k
    const float dy = a * (g01 - g00) + f.fr * (g11 - g10);  // dL/dy'_k
    sx += -dtk * dx;
    sy += -dtk * dy;
  }
  *gx = sx;
  *gy = sy;
}

__global__ void __launch_bounds__(256)
iwe_multiref_owner_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dt,
                              const int32_t* __restrict__ key_offsets, int32_t n, const float* __restrict__ flow, int H, int W,
                              int tile_h, int tile_w, int tiles_x, int64_t n_keys, int pad_h, int pad_w, Shifts shifts, int K,
                              const float* __restrict__ g_images, const float* __restrict__ affine, int g_lo, float* d_flow) {
  const int64_t hw = (int64_t)H * W;
  GradImages G;
  G.g = g_images;
  G.h = H + 2 * pad_h;
  G.w = W + 2 * pad_w;
  G.img = (int64_t)G.h * G.w;
  G.lo = g_lo;
#pragma unroll
  for (int k = 0; k < kMaxRef; ++k) {
    G.a[k] = (affine && k < K) ? affine[2 * k] : 1.0f;
    G.c[k] = (affine && k < K) ? affine[2 * k + 1] : 0.0f;
  }
  const int lane = threadIdx.x & (kWave - 1);
  // every lane of a wave stays to the end (the hot path shuffles): a key beyond the table or outside the image owns nothing
  const int64_t key = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t lin = -1;
  int32_t beg = 0, end = 0;
  if (key < n_keys) {
    const int tile_px = tile_h * tile_w;
    const int tile = (int)(key / tile_px), pit = (int)(key - (int64_t)tile * tile_px);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int r = ty * tile_h + pit / tile_w, c = tx * tile_w + pit % tile_w;
    if (r < H && c < W) {
      lin = (int64_t)r * W + c;
      beg = min(max(key_offsets[key], 0), n);  // a run never leaves the plan's events, whatever the table holds
      end = min(max(key_offsets[key + 1], beg), n);
    }
  }
  const int len = end - beg;
  const bool hot = lin >= 0 && len > kOwnerHot;
  if (lin >= 0 && !hot) {
    float sx = 0.0f, sy = 0.0f;
    if (len > 0) {
      const float u = flow[lin], v = flow[hw + lin];  // the run's one flow cell
      for (int32_t b0 = beg; b0 < end; b0 += kOwnerChunk) {
        float ex[kOwnerChunk], ey[kOwnerChunk], edt[kOwnerChunk];
        const int cnt = min(kOwnerChunk, end - b0);
#pragma unroll
        for (int j = 0; j < kOwnerChunk; ++j) {
          const bool live = j < cnt;
          ex[j] = live ? x[b0 + j] : 0.0f;
          ey[j] = live ? y[b0 + j] : 0.0f;
          edt[j] = live ? dt[b0 + j] : 0.0f;
        }
        for (int k = 0; k < K; ++k) {
          float g00[kOwnerChunk], g10[kOwnerChunk], g01[kOwnerChunk], g11[kOwnerChunk], fr[kOwnerChunk], fc[kOwnerChunk], dtk[kOwnerChunk];
#pragma unroll
          for (int j = 0; j < kOwnerChunk; ++j) {
            const bool live = j < cnt;
            dtk[j] = live ? edt[j] + shifts.at[k] : 0.0f;
            const Taps f = warped_taps(ex[j], ey[j], -dtk[j] * u, -dtk[j] * v, pad_h, pad_w);
            fr[j] = f.fr;
            fc[j] = f.fc;
            g00[j] = live ? G.at(k, f.R, f.C) : 0.0f;
            g10[j] = live ? G.at(k, f.R + 1, f.C) : 0.0f;
            g01[j] = live ? G.at(k, f.R, f.C + 1) : 0.0f;
            g11[j] = live ? G.at(k, f.R + 1, f.C + 1) : 0.0f;
          }
#pragma unroll
          for (int j = 0; j < kOwnerChunk; ++j) {
            const float a = 1.0f - fr[j], b = 1.0f - fc[j];
            const float dx = b * (g10[j] - g00[j]) + fc[j] * (g11[j] - g01[j]);  // dL/dx'_k
            const float dy = a * (g01[j] - g00[j]) + fr[j] * (g11[j] - g10[j]);  // dL/dy'_k
            sx += -dtk[j] * dx;  // (an unused slot: dt_k = 0 and every g = 0)
            sy += -dtk[j] * dy;
          }
        }
      }
    }
    d_flow[lin] = sx;  // consecutive lanes: consecutive columns of one image row
    d_flow[hw + lin] = sy;
  }
  // hot pixels of this wave, one after the other, all 64 lanes on each (every value that steers the loops is wave-uniform)
  unsigned long long hot_lanes = __ballot(hot);
  while (hot_lanes) {
    const int src = __ffsll((long long)hot_lanes) - 1;
    hot_lanes &= hot_lanes - 1;
    const int64_t hlin = __shfl(lin, src, kWave);
    const int32_t hbeg = __shfl(beg, src, kWave), hend = __shfl(end, src, kWave);
    const float u = flow[hlin], v = flow[hw + hlin];
    float ax = 0.0f, ay = 0.0f;
    for (int32_t base = hbeg; base < hend; base += kWave) {
      const int32_t i = base + lane;
      float gx = 0.0f, gy = 0.0f;
      if (i < hend) owner_event_grad(G, shifts, K, x[i], y[i], dt[i], u, v, pad_h, pad_w, &gx, &gy);
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) {  // butterfly: the same tree, and the same total, in every lane
        gx += __shfl_xor(gx, off, kWave);
        gy += __shfl_xor(gy, off, kWave);
      }
      ax += gx;
      ay += gy;
    }
    if (lane == 0) {
      d_flow[hlin] = ax;
      d_flow[hw + hlin] = ay;
    }
  }
}

// the checks the two entries share: K, the shifts (host memory), copied into the kernel argument
int read_shifts(const char* who, const float* shifts, int K, Shifts* out) {
  EBOS_REQUIRE(K >= 1 && K <= kMaxRef, "%s: K = %d is outside [1, %d]", who, K, kMaxRef);
  EBOS_REQUIRE(shifts != nullptr, "%s: shifts is NULL (a host array of K floats)", who);
  for (int k = 0; k < kMaxRef; ++k) out->at[k] = 0.0f;
  for (int k = 0; k < K; ++k) {
    EBOS_REQUIRE(std::isfinite(shifts[k]), "%s: shifts[%d] is not finite", who, k);
    out->at[k] = shifts[k];
  }
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

int ebos_iwe_multiref_fits(int tile_h, int tile_w, int halo, int K) {
  using namespace ebos;
  if (tile_h <= 0 || tile_w <= 0 || halo < 0 || !config_ok(kTiledConfigs, tile_h, tile_w, halo)) return 0;
  return fits_cells((size_t)(tile_h + 2 * halo) * (tile_w + 2 * halo), K);
}

int ebos_iwe_dense_multiref_tiled_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                      const float* flow, int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h,
                                      int pad_w, const float* shifts, int K, float* iwes, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(flow && iwes, "ebos_iwe_dense_multiref_tiled: NULL flow/iwes");
  EBOS_REQUIRE(key_offsets, "ebos_iwe_dense_multiref_tiled: key_offsets is NULL (the kernel needs a binned plan)");
  EBOS_REQUIRE((xs && ys && dts) || n == 0, "ebos_iwe_dense_multiref_tiled: NULL event buffer");
  Shifts sh;
  if (int rc = read_shifts("ebos_iwe_dense_multiref_tiled", shifts, K, &sh)) return rc;
  EBOS_REQUIRE(n >= 0 && n <= INT32_MAX && H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && pad_h >= 0 && pad_w >= 0 && splits >= 1 &&
                   splits <= 64,
               "ebos_iwe_dense_multiref_tiled: bad sizes (splits=%d)", splits);
  if (ebos_iwe_multiref_fits(tile_h, tile_w, halo, K) == 0) {
    set_error("ebos_iwe_dense_multiref_tiled: %d windows of tile %dx%d halo %d do not fit the LDS, or no kernel is built for it "
              "(see ebos_iwe_multiref_fits, ebos_tiled_config)", K, tile_h, tile_w, halo);
    return EBOS_ERR_UNSUPPORTED;
  }
  if (n == 0) return EBOS_OK;
  hipStream_t s = as_stream(stream);
  const int rc = dispatch_tiled(tile_h, tile_w, halo, [&](auto t) {
    return launch_multiref<t.th, t.tw, t.halo>(xs, ys, dts, key_offsets, (int32_t)n, flow, H, W, splits, pad_h, pad_w, sh, K, iwes, s);
  });
  if (rc == EBOS_ERR_UNSUPPORTED) {
    set_error("ebos_iwe_dense_multiref_tiled: no kernel built for tile %dx%d halo %d (see ebos_tiled_config)", tile_h, tile_w, halo);
    return rc;
  }
  if (rc != EBOS_OK) return rc;
  EBOS_CHECK_LAUNCH("ebos_iwe_dense_multiref_tiled");
  return EBOS_OK;
}

int ebos_iwe_dense_multiref_owner_bwd_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                          const float* flow, int H, int W, int tile_h, int tile_w, int pad_h, int pad_w,
                                          const float* shifts, int K, const float* g_images, const float* affine, int g_lo,
                                          float* d_flow, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(flow && g_images && d_flow, "ebos_iwe_dense_multiref_owner_bwd: NULL flow/g_images/d_flow");
  EBOS_REQUIRE(key_offsets, "ebos_iwe_dense_multiref_owner_bwd: key_offsets is NULL (the kernel needs a binned plan)");
  EBOS_REQUIRE((xs && ys && dts) || n == 0, "ebos_iwe_dense_multiref_owner_bwd: NULL event buffer");
  Shifts sh;
  if (int rc = read_shifts("ebos_iwe_dense_multiref_owner_bwd", shifts, K, &sh)) return rc;
  EBOS_REQUIRE(n >= 0 && n <= INT32_MAX && H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && pad_h >= 0 && pad_w >= 0 && g_lo >= 0,
               "ebos_iwe_dense_multiref_owner_bwd: bad sizes");
  const int tiles_y = (H + tile_h - 1) / tile_h, tiles_x = (W + tile_w - 1) / tile_w;
  const int64_t n_keys = (int64_t)tiles_y * tiles_x * tile_h * tile_w;
  EBOS_REQUIRE(n_keys < INT32_MAX, "ebos_iwe_dense_multiref_owner_bwd: %lld keys are more than a plan can hold", (long long)n_keys);
  // (n == 0 still runs: every cell is written, with zeros)
  iwe_multiref_owner_bwd_kernel<<<dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(
      xs, ys, dts, key_offsets, (int32_t)n, flow, H, W, tile_h, tile_w, tiles_x, n_keys, pad_h, pad_w, sh, K, g_images, affine, g_lo,
      d_flow);
  EBOS_CHECK_LAUNCH("ebos_iwe_dense_multiref_owner_bwd");
  return EBOS_OK;
}

}  // extern "C"
