// iwe_hvp.hip -- second-order pieces of the dense-flow contrast for gfx950 / CDNA4: the tangent image u = J v of the IWE along a
// flow direction v, and the Hessian-vector product of a cost that is quadratic in the image, summed by the owner of each source
// pixel's run.
//
//   warp     x' = x - dt * flow[0][pix];  y' = y - dt * flow[1][pix];  pix at (trunc x, trunc y);  taps and fractions (fr, fc) from
//            warped_taps.  Along v the warped position moves by (tx, ty) = (-dt * v[0][pix], -dt * v[1][pix]).
//   tangent  iwe_tangent_tiled_kernel: iwe_multiref_tiled_kernel of iwe_multiref.hip with one LDS window for u and, where the caller
//            wants it, a second one for the IWE itself.  The event is decoded once, flow and v are gathered once; the tangent's four
//            weights are the derivatives of the bilinear ones along (tx, ty) -- signed, they sum to zero.  Spill path, flush and the
//            "caller zero-fills the images" convention are that kernel's; f64 windows where they fit the LDS, else f32.
//   slab     the same kernel with another end (SLAB): every tile stores its window(s) to its slab of a workspace and
//            iwe_tangent_combine_kernel adds to every image cell the slabs that cover it, in tile order -- no float atomics but the
//            spill path's, so the bits repeat from call to call (where four tiles meet, the atomic flush adds three or more sums in
//            an order the hardware picks).
//   owner    iwe_hvp_owner_bwd_kernel: iwe_multiref_owner_bwd_kernel with two upstream images.  G1 = grad cost(IWE) gives the
//            gradient and the curvature of the bilinear weights (only their mixed second derivative is non-zero: `cross`);
//            G2 = grad cost(u) gives the Gauss-Newton part.  Per event
//                dx(G) = (1-fc)(G10-G00) + fc(G11-G01)      dy(G) = (1-fr)(G01-G00) + fr(G11-G10)
//                cross = G1_00 - G1_10 - G1_01 + G1_11
//                hv    += -dt * (dx(G2) + cross * ty,  dy(G2) + cross * tx)          d_flow += -dt * (dx(G1), dy(G1))
//            One lane owns a source pixel's run and is the only writer of its cells: no atomics, every cell written, the same bits on
//            every call.
#include <cmath>

#include "tile_configs.h"
#include "warp_footprint.h"

namespace ebos {
namespace {

constexpr size_t kLdsBytes = 160 * 1024;

// ---- tangent forward: one or two LDS-privatised windows per workgroup ----------------------------
constexpr int kTiledBlock = 1024;

template <int TH, int TW, int HALO, typename ACC, bool WITH_IWE, bool SLAB>
__global__ void __launch_bounds__(kTiledBlock)
iwe_tangent_tiled_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ dts,
                         const int32_t* __restrict__ key_offsets, int32_t n, const float* __restrict__ flow,
                         const float* __restrict__ dir, int H, int W, int tiles_x, int splits, int pad_h, int pad_w, float* iwe,
                         float* tangent, ACC* __restrict__ slab) {
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  constexpr int kWin = WITH_IWE ? 2 : 1;
  extern __shared__ double s_raw[];  // [kWin][LH][LW] of ACC: the tangent's window, then the IWE's
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

  for (int i = threadIdx.x; i < kWin * LH * LW; i += kTiledBlock) s_img[i] = ACC(0);
  __syncthreads();

  const int64_t hw = (int64_t)H * W;
  const int h = H + 2 * pad_h, w = W + 2 * pad_w;
  // LDS cell (0,0) <-> un-padded image pixel (oy, ox); padded pixel (oy + pad_h, ox + pad_w)
  const int oy = ty * TH - HALO, ox = tx * TW - HALO;

  // kUnroll events in flight per thread: the coalesced SoA loads first, then ONE gather of flow and v per event, then the LDS atomics
  constexpr int kUnroll = 4;
  for (int32_t base = my_beg + threadIdx.x; base < my_end; base += kTiledBlock * kUnroll) {
    float ex[kUnroll], ey[kUnroll], edt[kUnroll], fu[kUnroll], fv[kUnroll], du[kUnroll], dv[kUnroll];
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
      du[j] = live[j] ? dir[lin] : 0.0f;
      dv[j] = live[j] ? dir[hw + lin] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      if (!live[j]) continue;
      const Taps f = warped_taps(ex[j], ey[j], -edt[j] * fu[j], -edt[j] * fv[j], 0, 0);  // un-padded coordinates
      if (!f.ok) continue;
      const float fr = f.fr, fc = f.fc;
      const float a = 1.0f - fr, b = 1.0f - fc;
      const float tx_ = -edt[j] * du[j], ty_ = -edt[j] * dv[j];  // the warped position's tangent
      const float t00 = -b * tx_ - a * ty_, t10 = b * tx_ - fr * ty_;
      const float t01 = -fc * tx_ + a * ty_, t11 = fc * tx_ + fr * ty_;
      const float w00 = a * b, w10 = fr * b, w01 = a * fc, w11 = fr * fc;
      const int rl = f.R - oy, cl = f.C - ox;  // LDS cell of the top-left tap
      if (rl >= 0 && rl < LH - 1 && cl >= 0 && cl < LW - 1) {
        ACC* p = &s_img[rl * LW + cl];
        atomic_add(p, (ACC)t00);
        atomic_add(p + LW, (ACC)t10);
        atomic_add(p + 1, (ACC)t01);
        atomic_add(p + LW + 1, (ACC)t11);
        if constexpr (WITH_IWE) {
          ACC* q = p + LH * LW;
          atomic_add(q, (ACC)w00);
          atomic_add(q + LW, (ACC)w10);
          atomic_add(q + 1, (ACC)w01);
          atomic_add(q + LW + 1, (ACC)w11);
        }
      } else {
        // beyond the halo: straight to the images, so any displacement stays exact
        const int R = f.R + pad_h, C = f.C + pad_w;
        const bool rr0 = R >= 0 && R < h, rr1 = R + 1 >= 0 && R + 1 < h;
        const bool cc0 = C >= 0 && C < w, cc1 = C + 1 >= 0 && C + 1 < w;
        const int64_t gb = (int64_t)R * w + C;
        if (rr0 && cc0) atomic_add(&tangent[gb], t00);
        if (rr1 && cc0) atomic_add(&tangent[gb + w], t10);
        if (rr0 && cc1) atomic_add(&tangent[gb + 1], t01);
        if (rr1 && cc1) atomic_add(&tangent[gb + w + 1], t11);
        if constexpr (WITH_IWE) {
          if (rr0 && cc0) atomic_add(&iwe[gb], w00);
          if (rr1 && cc0) atomic_add(&iwe[gb + w], w10);
          if (rr0 && cc1) atomic_add(&iwe[gb + 1], w01);
          if (rr1 && cc1) atomic_add(&iwe[gb + w + 1], w11);
        }
      }
    }
  }
  __syncthreads();

  if constexpr (SLAB) {
    // the tile's window(s) as they are, zeros included, to the tile's slab: the combine pass sums the slabs that cover a cell in a
    // fixed order (one work item per tile on this route: splits == 1)
    ACC* out = slab + (size_t)tile * (kWin * LH * LW);
    for (int i = threadIdx.x; i < kWin * LH * LW; i += kTiledBlock) out[i] = s_img[i];
    return;
  }
  // flush: consecutive lanes -> consecutive columns of one image row, window after window
  const int gy0 = oy + pad_h, gx0 = ox + pad_w;
#pragma unroll
  for (int k = 0; k < kWin; ++k) {
    float* out = k == 0 ? tangent : iwe;
    const ACC* win = s_img + k * (LH * LW);
    for (int i = threadIdx.x; i < LH * LW; i += kTiledBlock) {
      const float v = (float)win[i];
      if (v == 0.0f) continue;
      const int rl = i / LW, cl = i - rl * LW;
      const int R = gy0 + rl, C = gx0 + cl;
      if (R >= 0 && R < h && C >= 0 && C < w) atomic_add(&out[(int64_t)R * w + C], v);
    }
  }
}

// ---- combine pass of the slab route: every image cell sums the slabs of the tiles whose window covers it, in tile order ---------
__device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

template <typename ACC>
__global__ void __launch_bounds__(256)
iwe_tangent_combine_kernel(const ACC* __restrict__ slab, const int32_t* __restrict__ key_offsets, int32_t n, int H, int W, int TH, int TW,
                           int HALO, int tiles_y, int tiles_x, int pad_h, int pad_w, int n_win, float* iwe, float* tangent) {
  const int h = H + 2 * pad_h, w = W + 2 * pad_w;
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= (int64_t)h * w) return;
  const int r = (int)(idx / w) - pad_h, c = (int)(idx % w) - pad_w;  // un-padded coordinates of this cell
  const int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  // window of tile ty covers rows [ty TH - HALO, ty TH + TH + HALO)
  const int ty_lo = max(0, -floor_div(-(r - TH - HALO + 1), TH)), ty_hi = min(tiles_y - 1, floor_div(r + HALO, TH));
  const int tx_lo = max(0, -floor_div(-(c - TW - HALO + 1), TW)), tx_hi = min(tiles_x - 1, floor_div(c + HALO, TW));
  double sum_t = 0.0, sum_i = 0.0;
  for (int ty = ty_lo; ty <= ty_hi; ++ty) {
    for (int tx = tx_lo; tx <= tx_hi; ++tx) {
      const int tile = ty * tiles_x + tx;
      const int32_t beg = min(max(key_offsets[tile * (TH * TW)], 0), n);
      const int32_t end = min(max(key_offsets[(tile + 1) * (TH * TW)], beg), n);
      if (beg == end) continue;  // a tile without events wrote no slab
      const int rl = r - (ty * TH - HALO), cl = c - (tx * TW - HALO);
      if (rl < 0 || rl >= LH || cl < 0 || cl >= LW) continue;
      const ACC* win = slab + (size_t)tile * ((size_t)n_win * LH * LW) + (size_t)rl * LW + cl;
      sum_t += (double)win[0];
      if (n_win == 2) sum_i += (double)win[(size_t)LH * LW];
    }
  }
  tangent[idx] += (float)sum_t;  // (on top of what the spill path added: the caller zero-filled the images)
  if (n_win == 2) iwe[idx] += (float)sum_i;
}

template <int TH, int TW, int HALO, typename ACC, bool WITH_IWE>
int launch_tangent_acc(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int32_t n, const float* flow,
                       const float* dir, int H, int W, int splits, int pad_h, int pad_w, float* iwe, float* tangent, void* slab,
                       hipStream_t s) {
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  constexpr size_t lds = (size_t)(WITH_IWE ? 2 : 1) * LH * LW * sizeof(ACC);
  static_assert(lds <= kLdsBytes, "the windows must fit the LDS");
  const int tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
  auto kern = slab ? iwe_tangent_tiled_kernel<TH, TW, HALO, ACC, WITH_IWE, true> : iwe_tangent_tiled_kernel<TH, TW, HALO, ACC, WITH_IWE, false>;
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      set_error("ebos_iwe_dense_tangent: cannot reserve %zu B of LDS", lds);
      return EBOS_ERR_LAUNCH;
    }
  }
  kern<<<dim3((unsigned)(tiles_y * tiles_x * splits)), dim3(kTiledBlock), lds, s>>>(xs, ys, dts, key_offsets, n, flow, dir, H, W, tiles_x,
                                                                                     splits, pad_h, pad_w, iwe, tangent, static_cast<ACC*>(slab));
  if (slab) {
    const int64_t cells = (int64_t)(H + 2 * pad_h) * (W + 2 * pad_w);
    iwe_tangent_combine_kernel<ACC><<<dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s>>>(
        static_cast<const ACC*>(slab), key_offsets, n, H, W, TH, TW, HALO, tiles_y, tiles_x, pad_h, pad_w, WITH_IWE ? 2 : 1, iwe, tangent);
  }
  return EBOS_OK;
}

// the accumulator of `fits` (ebos_iwe_multiref_fits of this triple with one or two windows): 2 = f64, 1 = f32
template <int TH, int TW, int HALO, bool WITH_IWE>
int launch_tangent(int fits, const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int32_t n, const float* flow,
                   const float* dir, int H, int W, int splits, int pad_h, int pad_w, float* iwe, float* tangent, void* slab, hipStream_t s) {
  constexpr size_t cells = (size_t)(TH + 2 * HALO) * (TW + 2 * HALO);
  constexpr size_t wins = WITH_IWE ? 2 : 1;
  if constexpr (cells * wins * sizeof(double) <= kLdsBytes) {
    if (fits == 2)
      return launch_tangent_acc<TH, TW, HALO, double, WITH_IWE>(xs, ys, dts, key_offsets, n, flow, dir, H, W, splits, pad_h, pad_w, iwe,
                                                                tangent, slab, s);
  }
  if constexpr (cells * wins * sizeof(float) <= kLdsBytes) {
    return launch_tangent_acc<TH, TW, HALO, float, WITH_IWE>(xs, ys, dts, key_offsets, n, flow, dir, H, W, splits, pad_h, pad_w, iwe,
                                                             tangent, slab, s);
  }
  return EBOS_ERR_UNSUPPORTED;
}

// what the two tangent entries share: the checks (before any HIP call) and the dispatch on the built triples; slab == NULL is the
// atomic flush
int tangent_entry(const char* who, const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                  const float* flow, const float* v, int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w,
                  bool want_slab, void* slab, size_t slab_bytes, float* iwe, float* tangent, ebos_stream_t stream) {
  EBOS_REQUIRE(flow && v && tangent, "%s: NULL flow/v/tangent", who);
  EBOS_REQUIRE(key_offsets, "%s: key_offsets is NULL (the kernel needs a binned plan)", who);
  EBOS_REQUIRE((xs && ys && dts) || n == 0, "%s: NULL event buffer", who);
  EBOS_REQUIRE(n >= 0 && n <= INT32_MAX && H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && pad_h >= 0 && pad_w >= 0 && splits >= 1 &&
                   splits <= 64,
               "%s: bad sizes (splits=%d)", who, splits);
  const int windows = iwe ? 2 : 1;
  const int fits = ebos_iwe_multiref_fits(tile_h, tile_w, halo, windows);
  if (fits == 0) {
    set_error("%s: %d window(s) of tile %dx%d halo %d do not fit the LDS, or no kernel is built for it (see ebos_iwe_multiref_fits, "
              "ebos_tiled_config)", who, windows, tile_h, tile_w, halo);
    return EBOS_ERR_UNSUPPORTED;
  }
  if (want_slab) {
    EBOS_REQUIRE(slab, "%s: workspace is NULL", who);
    const size_t need = ebos_iwe_tangent_slab_workspace_bytes(H, W, tile_h, tile_w, halo, windows);
    if (slab_bytes < need) {
      set_error("%s: workspace too small (%zu < %zu)", who, slab_bytes, need);
      return EBOS_ERR_SCRATCH;
    }
  }
  if (n == 0) return EBOS_OK;
  hipStream_t s = as_stream(stream);
  const int rc = dispatch_tiled(tile_h, tile_w, halo, [&](auto t) {
    return iwe ? launch_tangent<t.th, t.tw, t.halo, true>(fits, xs, ys, dts, key_offsets, (int32_t)n, flow, v, H, W, splits, pad_h, pad_w,
                                                          iwe, tangent, slab, s)
               : launch_tangent<t.th, t.tw, t.halo, false>(fits, xs, ys, dts, key_offsets, (int32_t)n, flow, v, H, W, splits, pad_h, pad_w,
                                                           nullptr, tangent, slab, s);
  });
  if (rc == EBOS_ERR_UNSUPPORTED) {
    set_error("%s: no kernel built for tile %dx%d halo %d (see ebos_tiled_config)", who, tile_h, tile_w, halo);
    return rc;
  }
  if (rc != EBOS_OK) return rc;
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

// ---- Hessian-vector product, pixel-owner form ----------------------------------------------------
// One lane per key walks its source pixel's run and is the only writer of that pixel's cells of hv (and of d_flow).
//   run <= kOwnerHot     kOwnerChunk events at a time: the events, then the eight taps of the chunk's events in flight together, added
//                        event by event -- the order is the plan's
//   longer (a hot pixel) the whole wave walks the run 64 events at a time; a butterfly sums the lanes (a fixed tree, the same total in
//                        every lane), added to the running sums
constexpr int kOwnerChunk = 4;
constexpr int kOwnerHot = 64;

struct TwoGradImages {
  const float* g1;  // [h, w]
  const float* g2;
  float a1, c1, a2, c2;  // G_i = a_i * g_i + c_i inside the valid region
  int h, w, lo;
  __device__ __forceinline__ bool in(int R, int C) const { return !(R < lo || R >= h - lo || C < lo || C >= w - lo); }
  __device__ __forceinline__ void at(int R, int C, float* v1, float* v2) const {
    if (!in(R, C)) {
      *v1 = 0.0f;
      *v2 = 0.0f;
      return;
    }
    const int64_t i = (int64_t)R * w + C;
    *v1 = a1 * g1[i] + c1;
    *v2 = a2 * g2[i] + c2;
  }
};

struct HvpSums {
  float hx, hy, gx, gy;
};

// one event's addends from its eight taps: p = G1, q = G2 at (00, 10, 01, 11)
__device__ __forceinline__ void hvp_event(float fr, float fc, float edt, float du, float dv, const float p[4], const float q[4], HvpSums* s) {
  const float a = 1.0f - fr, b = 1.0f - fc;
  const float dx1 = b * (p[1] - p[0]) + fc * (p[3] - p[2]);  // dL/dx'
  const float dy1 = a * (p[2] - p[0]) + fr * (p[3] - p[1]);  // dL/dy'
  const float dx2 = b * (q[1] - q[0]) + fc * (q[3] - q[2]);
  const float dy2 = a * (q[2] - q[0]) + fr * (q[3] - q[1]);
  const float cross = p[0] - p[1] - p[2] + p[3];
  const float tx = -edt * du, ty = -edt * dv;
  s->hx += -edt * (dx2 + cross * ty);
  s->hy += -edt * (dy2 + cross * tx);
  s->gx += -edt * dx1;
  s->gy += -edt * dy1;
}

__global__ void __launch_bounds__(256)
iwe_hvp_owner_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dt,
                         const int32_t* __restrict__ key_offsets, int32_t n, const float* __restrict__ flow,
                         const float* __restrict__ dir, int H, int W, int tile_h, int tile_w, int tiles_x, int64_t n_keys, int pad_h,
                         int pad_w, const float* __restrict__ g1, const float* __restrict__ g2, const float* __restrict__ affine, int g_lo,
                         float* d_flow, float* hv) {
  const int64_t hw = (int64_t)H * W;
  TwoGradImages G;
  G.g1 = g1;
  G.g2 = g2;
  G.h = H + 2 * pad_h;
  G.w = W + 2 * pad_w;
  G.lo = g_lo;
  G.a1 = affine ? affine[0] : 1.0f;
  G.c1 = affine ? affine[1] : 0.0f;
  G.a2 = affine ? affine[2] : 1.0f;
  G.c2 = affine ? affine[3] : 0.0f;
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
    HvpSums s = {0.0f, 0.0f, 0.0f, 0.0f};
    if (len > 0) {
      const float u = flow[lin], v = flow[hw + lin];      // the run's one flow cell ...
      const float du = dir[lin], dv = dir[hw + lin];      // ... and its one cell of the direction
      for (int32_t b0 = beg; b0 < end; b0 += kOwnerChunk) {
        float fr[kOwnerChunk], fc[kOwnerChunk], edt[kOwnerChunk], p[kOwnerChunk][4], q[kOwnerChunk][4];
        const int cnt = min(kOwnerChunk, end - b0);
#pragma unroll
        for (int j = 0; j < kOwnerChunk; ++j) {
          const bool live = j < cnt;
          const float ex = live ? x[b0 + j] : 0.0f, ey = live ? y[b0 + j] : 0.0f;
          edt[j] = live ? dt[b0 + j] : 0.0f;
          const Taps f = warped_taps(ex, ey, -edt[j] * u, -edt[j] * v, pad_h, pad_w);
          fr[j] = f.fr;
          fc[j] = f.fc;
          const int R = live ? f.R : -4, C = live ? f.C : -4;  // (a dead slot reads nothing: every tap 0, and dt = 0)
          G.at(R, C, &p[j][0], &q[j][0]);
          G.at(R + 1, C, &p[j][1], &q[j][1]);
          G.at(R, C + 1, &p[j][2], &q[j][2]);
          G.at(R + 1, C + 1, &p[j][3], &q[j][3]);
        }
#pragma unroll
        for (int j = 0; j < kOwnerChunk; ++j) hvp_event(fr[j], fc[j], edt[j], du, dv, p[j], q[j], &s);
      }
    }
    hv[lin] = s.hx;  // consecutive lanes: consecutive columns of one image row
    hv[hw + lin] = s.hy;
    if (d_flow) {
      d_flow[lin] = s.gx;
      d_flow[hw + lin] = s.gy;
    }
  }
  // hot pixels of this wave, one after the other, all 64 lanes on each (every value that steers the loops is wave-uniform)
  unsigned long long hot_lanes = __ballot(hot);
  while (hot_lanes) {
    const int src = __ffsll((long long)hot_lanes) - 1;
    hot_lanes &= hot_lanes - 1;
    const int64_t hlin = __shfl(lin, src, kWave);
    const int32_t hbeg = __shfl(beg, src, kWave), hend = __shfl(end, src, kWave);
    const float u = flow[hlin], v = flow[hw + hlin];
    const float du = dir[hlin], dv = dir[hw + hlin];
    HvpSums acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int32_t base = hbeg; base < hend; base += kWave) {
      const int32_t i = base + lane;
      HvpSums s = {0.0f, 0.0f, 0.0f, 0.0f};
      if (i < hend) {
        const float edt = dt[i];
        const Taps f = warped_taps(x[i], y[i], -edt * u, -edt * v, pad_h, pad_w);
        float p[4], q[4];
        G.at(f.R, f.C, &p[0], &q[0]);
        G.at(f.R + 1, f.C, &p[1], &q[1]);
        G.at(f.R, f.C + 1, &p[2], &q[2]);
        G.at(f.R + 1, f.C + 1, &p[3], &q[3]);
        hvp_event(f.fr, f.fc, edt, du, dv, p, q, &s);
      }
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) {  // butterfly: the same tree, and the same total, in every lane
        s.hx += __shfl_xor(s.hx, off, kWave);
        s.hy += __shfl_xor(s.hy, off, kWave);
        s.gx += __shfl_xor(s.gx, off, kWave);
        s.gy += __shfl_xor(s.gy, off, kWave);
      }
      acc.hx += s.hx;
      acc.hy += s.hy;
      acc.gx += s.gx;
      acc.gy += s.gy;
    }
    if (lane == 0) {
      hv[hlin] = acc.hx;
      hv[hw + hlin] = acc.hy;
      if (d_flow) {
        d_flow[hlin] = acc.gx;
        d_flow[hw + hlin] = acc.gy;
      }
    }
  }
}

}  // namespace
}  // namespace ebos

extern "C" {

size_t ebos_iwe_tangent_slab_workspace_bytes(int H, int W, int tile_h, int tile_w, int halo, int windows) {
  const int fits = (H > 0 && W > 0 && (windows == 1 || windows == 2)) ? ebos_iwe_multiref_fits(tile_h, tile_w, halo, windows) : 0;
  if (fits == 0) return 0;
  const size_t tiles = (size_t)((H + tile_h - 1) / tile_h) * ((W + tile_w - 1) / tile_w);
  return tiles * windows * (size_t)(tile_h + 2 * halo) * (tile_w + 2 * halo) * (fits == 2 ? sizeof(double) : sizeof(float));
}

int ebos_iwe_dense_tangent_tiled_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                     const float* flow, const float* v, int H, int W, int tile_h, int tile_w, int halo, int splits,
                                     int pad_h, int pad_w, float* iwe, float* tangent, ebos_stream_t stream) {
  return ebos::tangent_entry("ebos_iwe_dense_tangent_tiled", xs, ys, dts, key_offsets, n, flow, v, H, W, tile_h, tile_w, halo, splits,
                             pad_h, pad_w, false, nullptr, 0, iwe, tangent, stream);
}

int ebos_iwe_dense_tangent_slab_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                    const float* flow, const float* v, int H, int W, int tile_h, int tile_w, int halo, int pad_h,
                                    int pad_w, void* workspace, size_t workspace_bytes, float* iwe, float* tangent,
                                    ebos_stream_t stream) {
  return ebos::tangent_entry("ebos_iwe_dense_tangent_slab", xs, ys, dts, key_offsets, n, flow, v, H, W, tile_h, tile_w, halo, 1, pad_h,
                             pad_w, true, workspace, workspace_bytes, iwe, tangent, stream);
}

int ebos_iwe_dense_hvp_owner_bwd_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                     const float* flow, const float* v, int H, int W, int tile_h, int tile_w, int pad_h, int pad_w,
                                     const float* g1, const float* g2, const float* affine, int g_lo, float* d_flow, float* hv,
                                     ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(flow && v && g1 && g2 && hv, "ebos_iwe_dense_hvp_owner_bwd: NULL flow/v/g1/g2/hv");
  EBOS_REQUIRE(key_offsets, "ebos_iwe_dense_hvp_owner_bwd: key_offsets is NULL (the kernel needs a binned plan)");
  EBOS_REQUIRE((xs && ys && dts) || n == 0, "ebos_iwe_dense_hvp_owner_bwd: NULL event buffer");
  EBOS_REQUIRE(n >= 0 && n <= INT32_MAX && H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && pad_h >= 0 && pad_w >= 0 && g_lo >= 0,
               "ebos_iwe_dense_hvp_owner_bwd: bad sizes");
  const int tiles_y = (H + tile_h - 1) / tile_h, tiles_x = (W + tile_w - 1) / tile_w;
  const int64_t n_keys = (int64_t)tiles_y * tiles_x * tile_h * tile_w;
  EBOS_REQUIRE(n_keys < INT32_MAX, "ebos_iwe_dense_hvp_owner_bwd: %lld keys are more than a plan can hold", (long long)n_keys);
  // (n == 0 still runs: every cell is written, with zeros)
  iwe_hvp_owner_bwd_kernel<<<dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(
      xs, ys, dts, key_offsets, (int32_t)n, flow, v, H, W, tile_h, tile_w, tiles_x, n_keys, pad_h, pad_w, g1, g2, affine, g_lo, d_flow,
      hv);
  EBOS_CHECK_LAUNCH("ebos_iwe_dense_hvp_owner_bwd");
  return EBOS_OK;
}

}  // extern "C"
