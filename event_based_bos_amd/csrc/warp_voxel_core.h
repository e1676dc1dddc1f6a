// warp_voxel_core.h -- the device pieces the time-aware warp's translation units share: warp_voxel.hip (one reference time) and
// warp_voxel_multiref.hip (K reference times on the same voxel).  The general and the LDS-tiled forward body and the constants and
// run walk of the pixel-owner backward; the bilinear footprint and the upstream image of the backwards are warp_footprint.h's.
#pragma once
#include "warp_footprint.h"

namespace ebos {
namespace {

__device__ __forceinline__ int clamp_bin(uint8_t b, int T) { return min((int)b, T - 1); }

// general forward: any event order, four global float atomics per event (SHIFT as in the tiled body below)
template <bool SHIFT = false>
__device__ __forceinline__ void iwe_voxel_general_body(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dt,
                 const float* __restrict__ weight, const uint8_t* __restrict__ bins, int64_t n,
                 const float* __restrict__ voxel, int nbins, int H, int W, int row_stride, int pad_h, int pad_w, float* iwe,
                 float shift = 0.0f) {
  const int64_t hw = (int64_t)H * W;
  const int h = H + 2 * pad_h, w = W + 2 * pad_w;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float ex = x[i], ey = y[i], edt = (SHIFT && shift != 0.0f) ? dt[i] + shift : dt[i];
    if (!(ex > -1e9f && ex < 1e9f && ey > -1e9f && ey < 1e9f)) continue;
    const int64_t lin = (int64_t)(int)ex * row_stride + (int)ey;
    if (lin < 0 || lin >= hw) continue;  // torch.gather would raise (src/warp.py:334-336): dropped
    const float* f0 = voxel + (int64_t)clamp_bin(bins[i], nbins) * 2 * hw;
    const Taps f = warped_taps(ex, ey, -edt * f0[lin], -edt * f0[hw + lin], pad_h, pad_w);
    const float wv = weight ? weight[i] : 1.0f;
    const bool r0 = f.R >= 0 && f.R < h, r1 = f.R + 1 >= 0 && f.R + 1 < h;
    const bool c0 = f.C >= 0 && f.C < w, c1 = f.C + 1 >= 0 && f.C + 1 < w;
    const int64_t base = (int64_t)f.R * w + f.C;
    const float a = 1.0f - f.fr, b = 1.0f - f.fc;
    if (r0 && c0) atomic_add(&iwe[base], a * b * wv);
    if (r1 && c0) atomic_add(&iwe[base + w], f.fr * b * wv);
    if (r0 && c1) atomic_add(&iwe[base + 1], a * f.fc * wv);
    if (r1 && c1) atomic_add(&iwe[base + w + 1], f.fr * f.fc * wv);
  }
}

// tiled forward: LDS-privatised IWE tile per workgroup (iwe_dense_tiled_kernel with the bins as a fourth SoA stream; the
// accumulator rule -- f64 wherever tile + halo fits the LDS in doubles -- and the spill path beyond the halo are the same)
constexpr int kTiledBlock = 1024;

// the work item blockIdx.x = (tile, split) of ONE window: its offsets row, its voxel, its image
// SHIFT: the events' dt is dt + shift (another reference time, warp_voxel_multiref.hip); without it the body is the single
// reference's, to the instruction
template <int TH, int TW, int HALO, typename ACC, bool SHIFT = false>
__device__ __forceinline__ void iwe_voxel_tiled_body(ACC* s_img, const float* __restrict__ xs, const float* __restrict__ ys,
                                                     const float* __restrict__ dts, const float* __restrict__ weight,
                                                     const uint8_t* __restrict__ bins, const int32_t* __restrict__ key_offsets,
                                                     const float* __restrict__ voxel, int nbins, int H, int W, int tiles_x, int splits,
                                                     int pad_h, int pad_w, float* iwe, float shift = 0.0f) {
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  const int tile = blockIdx.x / splits, part = blockIdx.x - tile * splits;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int32_t beg = key_offsets[tile * (TH * TW)], end = key_offsets[(tile + 1) * (TH * TW)];
  if (beg == end) return;
  int32_t chunk = (end - beg + splits - 1) / splits;
  chunk = (chunk + kWave - 1) & ~(kWave - 1);
  const int32_t my_beg = beg + part * chunk;
  const int32_t my_end = min(end, my_beg + chunk);
  if (my_beg >= my_end) return;

  for (int i = threadIdx.x; i < LH * LW; i += kTiledBlock) s_img[i] = ACC(0);
  __syncthreads();

  const int64_t hw = (int64_t)H * W;
  const int h = H + 2 * pad_h, w = W + 2 * pad_w;
  // LDS cell (0,0) <-> un-padded image pixel (oy, ox); padded pixel (oy + pad_h, ox + pad_w)
  const int oy = ty * TH - HALO, ox = tx * TW - HALO;

  // kUnroll events in flight per thread: the coalesced SoA loads (bins among them) first, then the voxel gathers, then the LDS atomics
  constexpr int kUnroll = 8;
  for (int32_t base = my_beg + threadIdx.x; base < my_end; base += kTiledBlock * kUnroll) {
    float ex[kUnroll], ey[kUnroll], edt[kUnroll], wv[kUnroll], fu[kUnroll], fv[kUnroll];
    int kb[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int32_t i = base + k * kTiledBlock;
      const bool live = i < my_end;
      ex[k] = live ? xs[i] : -1.0f;  // -1 marks a dead slot
      ey[k] = live ? ys[i] : 0.0f;
      edt[k] = live ? dts[i] : 0.0f;
      kb[k] = live ? clamp_bin(bins[i], nbins) : 0;
      wv[k] = (live && weight) ? weight[i] : 1.0f;
      if (!live) wv[k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int32_t i = base + k * kTiledBlock;
      const int64_t lin = (int64_t)(int)ex[k] * W + (int)ey[k];  // binned events have a valid source pixel
      const bool live = i < my_end && lin >= 0 && lin < hw;
      const float* f0 = voxel + (int64_t)kb[k] * 2 * hw;
      fu[k] = live ? f0[lin] : 0.0f;
      fv[k] = live ? f0[hw + lin] : 0.0f;
      if (!live) wv[k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int32_t i = base + k * kTiledBlock;
      if (i >= my_end) break;
      const float d = (SHIFT && shift != 0.0f) ? edt[k] + shift : edt[k];  // (a zero shift: dt as it is)
      const Taps f = warped_taps(ex[k], ey[k], -d * fu[k], -d * fv[k], 0, 0);  // un-padded coordinates
      const float fr = f.fr, fc = f.fc;
      const float a = 1.0f - fr, b = 1.0f - fc;
      const float w00 = a * b * wv[k], w10 = fr * b * wv[k], w01 = a * fc * wv[k], w11 = fr * fc * wv[k];
      const int rl = f.R - oy, cl = f.C - ox;  // LDS cell of the top-left tap
      if (f.ok && rl >= 0 && rl < LH - 1 && cl >= 0 && cl < LW - 1) {
        ACC* p = &s_img[rl * LW + cl];
        atomic_add(p, (ACC)w00);
        atomic_add(p + LW, (ACC)w10);
        atomic_add(p + 1, (ACC)w01);
        atomic_add(p + LW + 1, (ACC)w11);
      } else if (f.ok) {
        // beyond the halo: straight to the image, so any displacement stays exact
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
  __syncthreads();

  // flush: consecutive lanes -> consecutive columns of one image row
  const int gy0 = oy + pad_h, gx0 = ox + pad_w;
  for (int i = threadIdx.x; i < LH * LW; i += kTiledBlock) {
    const float v = (float)s_img[i];
    if (v == 0.0f) continue;
    const int rl = i / LW, cl = i - rl * LW;
    const int R = gy0 + rl, C = gx0 + cl;
    if (R >= 0 && R < h && C >= 0 && C < w) atomic_add(&iwe[(int64_t)R * w + C], v);
  }
}

constexpr int kOwnerChunk = 8;
constexpr int kOwnerHot = 64;
constexpr int kOwnerSlots = 4;  // bins per lane of the hot path: 4 x 64 >= 255

// first event of each window in the concatenated streams, and the end of the last (a kernel argument: no table in memory)
// The run walk of the pixel-owner backwards (warp_voxel.hip: one reference time; warp_voxel_multiref.hip: K of them).  One window: its
// runs lie in [ev_lo, ev_hi) of the event arrays, and no run is followed outside that slice.  GRAD supplies the addends:
//   grad.chunk(lin, b0, cnt, kb, gx, gy)   events [b0, b0 + cnt) of source pixel `lin`, cnt <= kOwnerChunk: their bins (-1 in the unused
//                                          slots) and addends (0 there)
//   grad.event(lin, kb, i, &gx, &gy)       the addend of event i of source pixel `lin`, whose bin is kb
template <typename GRAD>
__device__ __forceinline__ void owner_bwd_walk(const GRAD& grad, const uint8_t* __restrict__ bins,
                                               const int32_t* __restrict__ key_offsets, int32_t ev_lo, int32_t ev_hi, int nbins, int H,
                                               int W, int tile_h, int tile_w, int tiles_x, int64_t n_keys, float* d_voxel) {
  const int64_t hw = (int64_t)H * W;
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
      beg = min(max(key_offsets[key], ev_lo), ev_hi);  // a run never leaves the window's events, whatever the table holds
      end = min(max(key_offsets[key + 1], beg), ev_hi);
    }
  }
  const int len = end - beg;
  const bool hot = lin >= 0 && len > kOwnerHot;
  if (lin >= 0 && !hot) {
    float* cell = d_voxel + lin;
    int kb[kOwnerChunk];
    float gx[kOwnerChunk], gy[kOwnerChunk];
    if (len <= kOwnerChunk) {
      grad.chunk(lin, beg, len, kb, gx, gy);
      for (int k = 0; k < nbins; ++k) {
        float sx = 0.0f, sy = 0.0f;
#pragma unroll
        for (int j = 0; j < kOwnerChunk; ++j)
          if (kb[j] == k) {
            sx += gx[j];
            sy += gy[j];
          }
        cell[(int64_t)(2 * k) * hw] = sx;  // consecutive lanes: consecutive columns of one image row
        cell[(int64_t)(2 * k + 1) * hw] = sy;
      }
    } else {
      for (int k = 0; k < 2 * nbins; ++k) cell[(int64_t)k * hw] = 0.0f;
      for (int32_t b0 = beg; b0 < end; b0 += kOwnerChunk) {
        grad.chunk(lin, b0, min(kOwnerChunk, end - b0), kb, gx, gy);
#pragma unroll
        for (int j = 0; j < kOwnerChunk; ++j)
          if (kb[j] >= 0) {
            cell[(int64_t)(2 * kb[j]) * hw] += gx[j];
            cell[(int64_t)(2 * kb[j] + 1) * hw] += gy[j];
          }
      }
    }
  }
  // hot pixels of this wave, one after the other, all 64 lanes on each (every value that steers the loops is wave-uniform)
  unsigned long long hot_lanes = __ballot(hot);
  while (hot_lanes) {
    const int src = __ffsll((long long)hot_lanes) - 1;
    hot_lanes &= hot_lanes - 1;
    const int64_t hlin = __shfl(lin, src, kWave);
    const int32_t hbeg = __shfl(beg, src, kWave), hend = __shfl(end, src, kWave);
    float ax[kOwnerSlots], ay[kOwnerSlots];  // lane l: the running sums of bins l, l + 64, l + 128, l + 192
#pragma unroll
    for (int s = 0; s < kOwnerSlots; ++s) ax[s] = ay[s] = 0.0f;
    for (int32_t base = hbeg; base < hend; base += kWave) {
      const int32_t i = base + lane;
      const bool live = i < hend;
      int kb = -1;
      float gx = 0.0f, gy = 0.0f;
      if (live) {
        kb = clamp_bin(bins[i], nbins);
        grad.event(hlin, kb, i, &gx, &gy);
      }
      unsigned long long todo = __ballot(live);
      while (todo) {  // one round per bin present in the chunk, in the order of the bins' first events
        const int k = __shfl(kb, __ffsll((long long)todo) - 1, kWave);
        const bool mine = live && kb == k;
        todo &= ~__ballot(mine);
        float sx = mine ? gx : 0.0f, sy = mine ? gy : 0.0f;
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {  // butterfly: the same tree, and the same total, in every lane
          sx += __shfl_xor(sx, off, kWave);
          sy += __shfl_xor(sy, off, kWave);
        }
        if (lane == (k & (kWave - 1))) {
#pragma unroll
          for (int s = 0; s < kOwnerSlots; ++s)
            if (s == (k >> 6)) {
              ax[s] += sx;
              ay[s] += sy;
            }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < kOwnerSlots; ++s) {
      const int k = s * kWave + lane;
      if (k < nbins) {
        d_voxel[(int64_t)(2 * k) * hw + hlin] = ax[s];
        d_voxel[(int64_t)(2 * k + 1) * hw + hlin] = ay[s];
      }
    }
  }
}

constexpr int kMaxWindows = EBOS_CMAX_VOXEL_MAX_BATCH;
struct WindowBases {
  int32_t at[kMaxWindows + 1];
};

bool bins_ok(int T) { return T >= 1 && T <= 255; }

}  // namespace
}  // namespace ebos
