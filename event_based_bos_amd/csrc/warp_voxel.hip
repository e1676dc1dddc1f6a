// warp_voxel.hip -- the time-aware warp for gfx950 / CDNA4: every event is displaced by the flow of ITS OWN time bin of a
// flow voxel [T, 2, H, W] (construct_dense_flow_voxel_* of flow_voxel.hip), materialised (A3 with a bin) and fused with the
// bilinear IWE and its backward (iwe_fused.hip with a bin).
//
//   bin      tau = (t - tmin) / (tmax - tmin) in float64 whatever the event type; k = min((int)(tau * T), T - 1); tmax == tmin -> 0
//   warp     i = trunc(x) * row_stride + trunc(y);  x' = x - dt * V[k][0][i];  y' = y - dt * V[k][1][i];  t' = dt;  p' = p
//            (dt and the operation order exactly as warp_kernels.hip: src/warp.py:283-287, 330-337, no FMA contraction)
//   fused    iwe_dense_kernel / iwe_dense_tiled_kernel / iwe_dense_bwd_kernel of iwe_fused.hip with the gather
//            V[(k * 2 + c) * H * W + lin] and the bins as one more SoA stream (1 B/event)
//   owner    iwe_voxel_owner_bwd_kernel: the backward for a binned plan, summed by the owner of each source pixel's run -- no
//            atomics, every cell of d_voxel written, the same bits on every call
//   batch    iwe_voxel_tiled_batch_kernel / iwe_voxel_owner_bwd_batch_kernel: the tiled forward and the owner backward for several
//            windows of one geometry, the window an outer grid dimension (blockIdx.y) over a stacked plan; the single kernels' bodies
//
// Every kernel reads a bin as min(bins[i], T - 1): a bins array that was made for another T cannot index outside the voxel.
// Dead and padding slots never gather.
#include "tile_configs.h"
#include "warp_voxel_core.h"

namespace ebos {
namespace {

// ---- AoS helpers (as warp_kernels.hip) -----------------------------------------------------------
template <typename T>
struct Vec4;
template <>
struct Vec4<float> {
  using type = float4;
};
template <>
struct Vec4<double> {
  using type = double4;
};
template <typename T>
__device__ __forceinline__ typename Vec4<T>::type load_event(const T* base, int64_t i) {
  return reinterpret_cast<const typename Vec4<T>::type*>(base)[i];
}
template <typename T>
__device__ __forceinline__ void store_event(T* base, int64_t i, typename Vec4<T>::type v) {
  reinterpret_cast<typename Vec4<T>::type*>(base)[i] = v;
}

template <typename T>
__device__ __forceinline__ T event_dt(T t, const TimeBase<T>& tb, int normalize_t) {
#pragma clang fp contract(off)
  T dt = t - tb.ref;                    // src/warp.py:283
  if (normalize_t) dt = dt / tb.period;  // :284-287
  return dt;
}

// source-pixel linear index of src/warp.py:334 (trunc toward zero, flattened bounds as torch.gather)
template <typename T>
__device__ __forceinline__ bool source_index(T x, T y, int row_stride, int64_t hw, int64_t* lin) {
  const T lim = T(1e15);
  if (!(x > -lim && x < lim && y > -lim && y < lim)) return false;  // NaN / Inf
  const int64_t l = static_cast<int64_t>(x) * row_stride + static_cast<int64_t>(y);
  *lin = l;
  return l >= 0 && l < hw;
}


// ---- the bin rule, in float64 --------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
time_bins_kernel(const T* __restrict__ events, const T* __restrict__ tminmax, int64_t n, int nbins,
                 uint8_t* __restrict__ bins) {
#pragma clang fp contract(off)
  const int64_t row = blockIdx.y;
  const T* ev = events + row * n * 4;
  uint8_t* out = bins + row * n;
  const double tmin = (double)tminmax[2 * row], tmax = (double)tminmax[2 * row + 1];  // float -> double is exact
  const double span = tmax - tmin;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int k = 0;
    if (span > 0.0) {
      const double tau = ((double)ev[4 * i + 2] - tmin) / span;
      const double s = tau * (double)nbins;
      if (s >= (double)nbins) k = nbins - 1;  // t == tmax (and anything later, were tminmax not this window's)
      else if (s > 0.0) k = (int)s;           // NaN and negatives stay in bin 0
    }
    out[i] = (uint8_t)k;
  }
}

// ---- materialised warp, forward ------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
warp_voxel_kernel(const T* __restrict__ events, const T* __restrict__ voxel, const T* __restrict__ tminmax, int ref_mode,
                  double ref_fraction, int normalize_t, int64_t n, int nbins, int H, int W, int row_stride,
                  const uint8_t* __restrict__ bins, T* __restrict__ warped, int32_t* oob_count) {
#pragma clang fp contract(off)
  const int64_t row = blockIdx.y;
  const int64_t hw = (int64_t)H * W;
  const T* ev = events + row * n * 4;
  const T* vx = voxel + row * nbins * 2 * hw;
  const uint8_t* bn = bins + row * n;
  T* out = warped + row * n * 4;
  const TimeBase<T> tb = time_base(tminmax + 2 * row, ref_mode, ref_fraction);
  int bad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    auto e = load_event(ev, i);
    const T dt = event_dt(e.z, tb, normalize_t);
    int64_t lin;
    if (source_index(e.x, e.y, row_stride, hw, &lin)) {
      const T* f0 = vx + (int64_t)clamp_bin(bn[i], nbins) * 2 * hw;
      const T u = f0[lin], v = f0[hw + lin];
      const T du = dt * u, dv = dt * v;  // separate roundings: mul, then sub (src/warp.py:335-336)
      e.x = e.x - du;
      e.y = e.y - dv;
    } else {
      ++bad;
    }
    e.z = dt;
    store_event(out, i, e);
  }
  if (oob_count != nullptr && bad) atomicAdd(oob_count, bad);
}

// ---- materialised warp, backward: d_voxel[k][c][src] += -dt * d_warped[c] ------------------------
template <typename T>
__global__ void __launch_bounds__(256)
warp_voxel_bwd_kernel(const T* __restrict__ events, const T* __restrict__ tminmax, int ref_mode, double ref_fraction,
                      int normalize_t, const T* __restrict__ d_warped, int64_t n, int nbins, int H, int W, int row_stride,
                      const uint8_t* __restrict__ bins, T* d_voxel) {
  const int64_t row = blockIdx.y;
  const int64_t hw = (int64_t)H * W;
  const T* ev = events + row * n * 4;
  const T* dw = d_warped + row * n * 4;
  const uint8_t* bn = bins + row * n;
  T* gv = d_voxel + row * nbins * 2 * hw;
  const TimeBase<T> tb = time_base(tminmax + 2 * row, ref_mode, ref_fraction);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const auto e = load_event(ev, i);
    const auto g = load_event(dw, i);
    const T dt = event_dt(e.z, tb, normalize_t);
    int64_t lin;
    if (source_index(e.x, e.y, row_stride, hw, &lin)) {
      T* g0 = gv + (int64_t)clamp_bin(bn[i], nbins) * 2 * hw;
      atomic_add(&g0[lin], -dt * g.x);
      atomic_add(&g0[hw + lin], -dt * g.y);
    }
  }
}

// ---- fused warp + IWE ----------------------------------------------------------------------------

// general forward: any event order, four global float atomics per event
__global__ void __launch_bounds__(256)
iwe_voxel_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dt,
                 const float* __restrict__ weight, const uint8_t* __restrict__ bins, int64_t n,
                 const float* __restrict__ voxel, int nbins, int H, int W, int row_stride, int pad_h, int pad_w, float* iwe) {
  iwe_voxel_general_body(x, y, dt, weight, bins, n, voxel, nbins, H, W, row_stride, pad_h, pad_w, iwe);
}

template <int TH, int TW, int HALO, typename ACC>
__global__ void __launch_bounds__(kTiledBlock)
iwe_voxel_tiled_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ dts,
                       const float* __restrict__ weight, const uint8_t* __restrict__ bins,
                       const int32_t* __restrict__ key_offsets, const float* __restrict__ voxel, int nbins, int H, int W,
                       int tiles_x, int splits, int pad_h, int pad_w, float* iwe) {
  extern __shared__ double s_raw[];  // [LH][LW] of ACC
  iwe_voxel_tiled_body<TH, TW, HALO, ACC>(reinterpret_cast<ACC*>(s_raw), xs, ys, dts, weight, bins, key_offsets, voxel, nbins, H, W,
                                          tiles_x, splits, pad_h, pad_w, iwe);
}

// several windows of one geometry: blockIdx.y is the window.  The event streams are the windows' streams one after the other and
// row b of key_offsets [B, n_keys + 1] holds window b's offsets INTO THE CONCATENATION, so a window is found without a pointer table.
template <int TH, int TW, int HALO, typename ACC>
__global__ void __launch_bounds__(kTiledBlock)
iwe_voxel_tiled_batch_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ dts,
                             const uint8_t* __restrict__ bins, const int32_t* __restrict__ key_offsets,
                             const float* __restrict__ voxel, int nbins, int H, int W, int tiles_x, int tiles_y, int splits, int pad_h,
                             int pad_w, float* iwe) {
  extern __shared__ double s_raw[];  // [LH][LW] of ACC
  const int64_t b = blockIdx.y;
  const int64_t n_keys = (int64_t)tiles_y * tiles_x * (TH * TW);
  iwe_voxel_tiled_body<TH, TW, HALO, ACC>(reinterpret_cast<ACC*>(s_raw), xs, ys, dts, nullptr, bins, key_offsets + b * (n_keys + 1),
                                          voxel + b * nbins * 2 * (int64_t)H * W, nbins, H, W, tiles_x, splits, pad_h, pad_w,
                                          iwe + b * (int64_t)(H + 2 * pad_h) * (W + 2 * pad_w));
}


template <int TH, int TW, int HALO>
int launch_voxel_tiled(const float* xs, const float* ys, const float* dts, const float* weight, const uint8_t* bins,
                       const int32_t* key_offsets, const float* voxel, int nbins, int H, int W, int splits, int pad_h,
                       int pad_w, float* iwe, hipStream_t s) {
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  using ACC = typename TileAcc<TH, TW, HALO>::type;
  constexpr size_t lds = (size_t)LH * LW * sizeof(ACC);
  static_assert(lds <= 160 * 1024, "tile + halo must fit the 160 KiB LDS of a CDNA4 CU");
  const int tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
  auto kern = iwe_voxel_tiled_kernel<TH, TW, HALO, ACC>;
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess) {
      set_error("ebos_iwe_voxel_tiled: cannot reserve %zu B of LDS", lds);
      return EBOS_ERR_LAUNCH;
    }
  }
  kern<<<dim3((unsigned)(tiles_y * tiles_x * splits)), dim3(kTiledBlock), lds, s>>>(
      xs, ys, dts, weight, bins, key_offsets, voxel, nbins, H, W, tiles_x, splits, pad_h, pad_w, iwe);
  return EBOS_OK;
}

template <int TH, int TW, int HALO>
int launch_voxel_tiled_batch(const float* xs, const float* ys, const float* dts, const uint8_t* bins, const int32_t* key_offsets,
                             int B, const float* voxel, int nbins, int H, int W, int splits, int pad_h, int pad_w, float* iwe,
                             hipStream_t s) {
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  using ACC = typename TileAcc<TH, TW, HALO>::type;
  constexpr size_t lds = (size_t)LH * LW * sizeof(ACC);
  const int tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
  auto kern = iwe_voxel_tiled_batch_kernel<TH, TW, HALO, ACC>;
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess) {
      set_error("ebos_iwe_voxel_tiled_batch: cannot reserve %zu B of LDS", lds);
      return EBOS_ERR_LAUNCH;
    }
  }
  kern<<<dim3((unsigned)(tiles_y * tiles_x * splits), (unsigned)B), dim3(kTiledBlock), lds, s>>>(
      xs, ys, dts, bins, key_offsets, voxel, nbins, H, W, tiles_x, tiles_y, splits, pad_h, pad_w, iwe);
  return EBOS_OK;
}

// ---- fused backward ------------------------------------------------------------------------------

template <bool SORTED>
__global__ void __launch_bounds__(256)
iwe_voxel_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dt,
                     const float* __restrict__ weight, const uint8_t* __restrict__ bins, int64_t n,
                     const float* __restrict__ voxel, int nbins, int H, int W, int row_stride, int pad_h, int pad_w,
                     const float* __restrict__ g_image, const float* __restrict__ affine, int g_lo, float* d_voxel,
                     float* __restrict__ d_weight) {
  const int64_t hw = (int64_t)H * W;
  GradImage G;
  G.g = g_image;
  G.a = affine ? affine[0] : 1.0f;
  G.c = affine ? affine[1] : 0.0f;
  G.h = H + 2 * pad_h;
  G.w = W + 2 * pad_w;
  G.lo = g_lo;
  const int lane = threadIdx.x & (kWave - 1);
  // whole waves iterate together so that the shuffles below see all 64 lanes
  const int64_t n_round = (n + kWave - 1) / kWave * kWave;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t key = -1;  // k * H * W + lin names the pair of d_voxel cells this event adds to
    int kb = 0;
    float gx = 0.0f, gy = 0.0f;
    if (i < n) {
      const float ex = x[i], ey = y[i], edt = dt[i];
      int64_t lin = -1;
      if (ex > -1e9f && ex < 1e9f && ey > -1e9f && ey < 1e9f) {
        lin = (int64_t)(int)ex * row_stride + (int)ey;
        if (lin < 0 || lin >= hw) lin = -1;
      }
      if (lin >= 0) {
        kb = clamp_bin(bins[i], nbins);
        const float* f0 = voxel + (int64_t)kb * 2 * hw;
        const Taps f = warped_taps(ex, ey, -edt * f0[lin], -edt * f0[hw + lin], pad_h, pad_w);
        const float g00 = G.at(f.R, f.C), g10 = G.at(f.R + 1, f.C);
        const float g01 = G.at(f.R, f.C + 1), g11 = G.at(f.R + 1, f.C + 1);
        const float wv = weight ? weight[i] : 1.0f;
        const float a = 1.0f - f.fr, b = 1.0f - f.fc;
        const float dx = wv * (b * (g10 - g00) + f.fc * (g11 - g01));  // dL/dx'
        const float dy = wv * (a * (g01 - g00) + f.fr * (g11 - g10));  // dL/dy'
        gx = -edt * dx;                                                // dL/dV[k][0][src]
        gy = -edt * dy;
        key = (int64_t)kb * hw + lin;
        if (d_weight) d_weight[i] = a * b * g00 + f.fr * b * g10 + a * f.fc * g01 + f.fr * f.fc * g11;
      } else if (d_weight) {
        d_weight[i] = 0.0f;
      }
    }
    const int64_t cell = key >= 0 ? key + (int64_t)kb * hw : 0;  // (k * 2 + 0) * H * W + lin
    if (SORTED) {
      // events of one source pixel are contiguous, in whatever order of their bins: the segmented wave reduction keys on
      // (bin, pixel), so a run is a stretch of neighbours that add to the same cells -- one atomic pair per run
      const int64_t prev = __shfl_up(key, 1, kWave);
      const bool head = (lane == 0) || (prev != key);
      const unsigned long long heads = __ballot(head);
      const int run = __popcll(heads & (~0ull >> (63 - lane)));  // number of heads at or below this lane
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const float ox_ = __shfl_down(gx, off, kWave);
        const float oy_ = __shfl_down(gy, off, kWave);
        const int orun = __shfl_down(run, off, kWave);
        if (lane + off < kWave && orun == run) {
          gx += ox_;
          gy += oy_;
        }
      }
      if (head && key >= 0) {
        atomic_add(&d_voxel[cell], gx);
        atomic_add(&d_voxel[cell + hw], gy);
      }
    } else if (key >= 0) {
      atomic_add(&d_voxel[cell], gx);
      atomic_add(&d_voxel[cell + hw], gy);
    }
  }
}

// ---- fused backward, pixel-owner form ------------------------------------------------------------
// A cell d_voxel[k][c][i] receives addends only from events whose SOURCE pixel is i, and a binned plan keeps the events of one
// source pixel in one run (key_offsets).  One lane per key walks its pixel's run and is the only writer of that pixel's 2 T cells:
// no atomics, every cell written (zeros where nothing lands), the order of the additions fixed by the plan -> the same bits on
// every call.  Keys of an overhanging tile's pixels outside the image own no cell.
//   Runs are walked kOwnerChunk events at a time, in stages, so that a lane's loads are in flight together instead of one event's
//   chain after the other: the events, then the voxel gathers, then the four taps of each, then the arithmetic.
//   run <= kOwnerChunk   the addends stay in registers; each cell is stored once, the sum of the run's events of that bin in run order
//   run <= kOwnerHot     the lane zeroes its cells and adds chunk after chunk, event by event (plain loads and stores of cells
//                        nobody else touches)
//   longer (a hot pixel) the whole wave walks the run 64 events at a time; per chunk and per bin present in it, a butterfly sum
//                        over the lanes (a fixed tree), added to the bin's running sum, which lane (k mod 64) keeps in registers

// the addend of iwe_voxel_bwd_kernel for one event of source pixel `lin` and bin `kb`
__device__ __forceinline__ void owner_event_grad(const GradImage& G, const float* __restrict__ voxel, int64_t hw, int64_t lin, int kb,
                                                 float ex, float ey, float edt, float wv, int pad_h, int pad_w, float* gx, float* gy) {
  const float* f0 = voxel + (int64_t)kb * 2 * hw;
  const Taps f = warped_taps(ex, ey, -edt * f0[lin], -edt * f0[hw + lin], pad_h, pad_w);
  const float g00 = G.at(f.R, f.C), g10 = G.at(f.R + 1, f.C);
  const float g01 = G.at(f.R, f.C + 1), g11 = G.at(f.R + 1, f.C + 1);
  const float a = 1.0f - f.fr, b = 1.0f - f.fc;
  const float dx = wv * (b * (g10 - g00) + f.fc * (g11 - g01));  // dL/dx'
  const float dy = wv * (a * (g01 - g00) + f.fr * (g11 - g10));  // dL/dy'
  *gx = -edt * dx;
  *gy = -edt * dy;
}

// events [b0, b0 + cnt) of source pixel `lin`, cnt <= kOwnerChunk: their bins (-1 in the unused slots) and addends (0 there)
__device__ __forceinline__ void owner_chunk(const GradImage& G, const float* __restrict__ x, const float* __restrict__ y,
                                            const float* __restrict__ dt, const float* __restrict__ weight,
                                            const uint8_t* __restrict__ bins, const float* __restrict__ voxel, int nbins, int64_t hw,
                                            int64_t lin, int32_t b0, int cnt, int pad_h, int pad_w, int (&kb)[kOwnerChunk],
                                            float (&gx)[kOwnerChunk], float (&gy)[kOwnerChunk]) {
  float ex[kOwnerChunk], ey[kOwnerChunk], edt[kOwnerChunk], fu[kOwnerChunk], fv[kOwnerChunk];
#pragma unroll
  for (int j = 0; j < kOwnerChunk; ++j) {
    const bool live = j < cnt;
    const int32_t i = b0 + j;
    kb[j] = live ? clamp_bin(bins[i], nbins) : -1;
    ex[j] = live ? x[i] : 0.0f;
    ey[j] = live ? y[i] : 0.0f;
    edt[j] = live ? dt[i] : 0.0f;
  }
#pragma unroll
  for (int j = 0; j < kOwnerChunk; ++j) {
    const bool live = j < cnt;
    const float* f0 = voxel + (int64_t)(live ? kb[j] : 0) * 2 * hw;
    fu[j] = live ? f0[lin] : 0.0f;
    fv[j] = live ? f0[hw + lin] : 0.0f;
  }
  float g00[kOwnerChunk], g10[kOwnerChunk], g01[kOwnerChunk], g11[kOwnerChunk], fr[kOwnerChunk], fc[kOwnerChunk];
#pragma unroll
  for (int j = 0; j < kOwnerChunk; ++j) {
    const bool live = j < cnt;
    const Taps f = warped_taps(ex[j], ey[j], -edt[j] * fu[j], -edt[j] * fv[j], pad_h, pad_w);
    fr[j] = f.fr;
    fc[j] = f.fc;
    g00[j] = live ? G.at(f.R, f.C) : 0.0f;
    g10[j] = live ? G.at(f.R + 1, f.C) : 0.0f;
    g01[j] = live ? G.at(f.R, f.C + 1) : 0.0f;
    g11[j] = live ? G.at(f.R + 1, f.C + 1) : 0.0f;
  }
#pragma unroll
  for (int j = 0; j < kOwnerChunk; ++j) {
    const float wv = (weight != nullptr && j < cnt) ? weight[b0 + j] : 1.0f;
    const float a = 1.0f - fr[j], b = 1.0f - fc[j];
    const float dx = wv * (b * (g10[j] - g00[j]) + fc[j] * (g11[j] - g01[j]));  // dL/dx'
    const float dy = wv * (a * (g01[j] - g00[j]) + fr[j] * (g11[j] - g10[j]));  // dL/dy'
    gx[j] = -edt[j] * dx;  // (an unused slot: edt = 0 and every g = 0)
    gy[j] = -edt[j] * dy;
  }
}

// the addends of one reference time: the plan's own dt
struct SingleGrad {
  GradImage G;
  const float* __restrict__ x;
  const float* __restrict__ y;
  const float* __restrict__ dt;
  const float* __restrict__ weight;
  const uint8_t* __restrict__ bins;
  const float* __restrict__ voxel;
  int nbins, pad_h, pad_w;
  int64_t hw;
  __device__ __forceinline__ void chunk(int64_t lin, int32_t b0, int cnt, int (&kb)[kOwnerChunk], float (&gx)[kOwnerChunk],
                                        float (&gy)[kOwnerChunk]) const {
    owner_chunk(G, x, y, dt, weight, bins, voxel, nbins, hw, lin, b0, cnt, pad_h, pad_w, kb, gx, gy);
  }
  __device__ __forceinline__ void event(int64_t lin, int kb, int32_t i, float* gx, float* gy) const {
    owner_event_grad(G, voxel, hw, lin, kb, x[i], y[i], dt[i], weight ? weight[i] : 1.0f, pad_h, pad_w, gx, gy);
  }
};

// one window: its runs lie in [ev_lo, ev_hi) of the event arrays (owner_bwd_walk, warp_voxel_core.h)
__device__ __forceinline__ void iwe_voxel_owner_bwd_body(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ dt, const float* __restrict__ weight,
                                                         const uint8_t* __restrict__ bins, const int32_t* __restrict__ key_offsets,
                                                         int32_t ev_lo, int32_t ev_hi, const float* __restrict__ voxel, int nbins, int H,
                                                         int W, int tile_h, int tile_w, int tiles_x, int64_t n_keys, int pad_h,
                                                         int pad_w, const float* __restrict__ g_image,
                                                         const float* __restrict__ affine, int g_lo, float* d_voxel) {
  SingleGrad grad;
  grad.G.g = g_image;
  grad.G.a = affine ? affine[0] : 1.0f;
  grad.G.c = affine ? affine[1] : 0.0f;
  grad.G.h = H + 2 * pad_h;
  grad.G.w = W + 2 * pad_w;
  grad.G.lo = g_lo;
  grad.x = x, grad.y = y, grad.dt = dt, grad.weight = weight, grad.bins = bins, grad.voxel = voxel;
  grad.nbins = nbins, grad.pad_h = pad_h, grad.pad_w = pad_w, grad.hw = (int64_t)H * W;
  owner_bwd_walk(grad, bins, key_offsets, ev_lo, ev_hi, nbins, H, W, tile_h, tile_w, tiles_x, n_keys, d_voxel);
}

__global__ void __launch_bounds__(256)
iwe_voxel_owner_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dt,
                           const float* __restrict__ weight, const uint8_t* __restrict__ bins,
                           const int32_t* __restrict__ key_offsets, int32_t n, const float* __restrict__ voxel, int nbins, int H,
                           int W, int tile_h, int tile_w, int tiles_x, int64_t n_keys, int pad_h, int pad_w,
                           const float* __restrict__ g_image, const float* __restrict__ affine, int g_lo, float* d_voxel) {
  iwe_voxel_owner_bwd_body(x, y, dt, weight, bins, key_offsets, 0, n, voxel, nbins, H, W, tile_h, tile_w, tiles_x, n_keys, pad_h, pad_w,
                           g_image, affine, g_lo, d_voxel);
}


// several windows: the key is (pixel key, window = blockIdx.y); window b owns row b of the offsets, voxel[b], g_image[b], affine[b]
// and d_voxel[b]
__global__ void __launch_bounds__(256)
iwe_voxel_owner_bwd_batch_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dt,
                                 const uint8_t* __restrict__ bins, const int32_t* __restrict__ key_offsets, WindowBases bases,
                                 const float* __restrict__ voxel, int nbins, int H, int W, int tile_h, int tile_w, int tiles_x,
                                 int64_t n_keys, int pad_h, int pad_w, const float* __restrict__ g_image,
                                 const float* __restrict__ affine, int g_lo, float* d_voxel) {
  const int b = blockIdx.y;
  const int64_t cells = (int64_t)nbins * 2 * H * W;
  iwe_voxel_owner_bwd_body(x, y, dt, nullptr, bins, key_offsets + (int64_t)b * (n_keys + 1), bases.at[b], bases.at[b + 1],
                           voxel + b * cells, nbins, H, W, tile_h, tile_w, tiles_x, n_keys, pad_h, pad_w,
                           g_image + (int64_t)b * (H + 2 * pad_h) * (W + 2 * pad_w), affine ? affine + 2 * b : nullptr, g_lo,
                           d_voxel + b * cells);
}

bool ref_mode_ok(int m) { return m >= EBOS_REF_FIRST && m <= EBOS_REF_TIMEBASE; }

template <typename T>
int time_bins_impl(const T* events, const T* tminmax, int64_t b, int64_t n, int nbins, uint8_t* bins, ebos_stream_t stream) {
  EBOS_REQUIRE(tminmax != nullptr, "ebos_event_time_bins: tminmax is NULL");
  EBOS_REQUIRE((events && bins) || n == 0, "ebos_event_time_bins: NULL events/bins");
  EBOS_REQUIRE(bins_ok(nbins), "ebos_event_time_bins: T = %d is outside [1, 255]", nbins);
  EBOS_REQUIRE(b >= 1 && b <= 65535 && n >= 0, "ebos_event_time_bins: bad sizes b=%lld n=%lld", (long long)b, (long long)n);
  if (n == 0) return EBOS_OK;
  dim3 grid(stream_grid(n, 256), (unsigned)b);
  time_bins_kernel<T><<<grid, dim3(256), 0, as_stream(stream)>>>(events, tminmax, n, nbins, bins);
  EBOS_CHECK_LAUNCH("ebos_event_time_bins");
  return EBOS_OK;
}

template <typename T>
int warp_voxel_impl(const T* events, const T* voxel, const T* tminmax, int ref_mode, double ref_fraction, int normalize_t,
                    int64_t b, int64_t n, int nbins, int H, int W, int row_stride, const uint8_t* bins, T* warped,
                    int32_t* oob_count, ebos_stream_t stream) {
  EBOS_REQUIRE(voxel && tminmax, "ebos_warp_voxel: NULL voxel/tminmax");
  EBOS_REQUIRE((events && warped && bins) || n == 0, "ebos_warp_voxel: NULL events/warped/bins");
  EBOS_REQUIRE(ref_mode_ok(ref_mode), "ebos_warp_voxel: bad ref_mode %d", ref_mode);
  EBOS_REQUIRE(bins_ok(nbins), "ebos_warp_voxel: T = %d is outside [1, 255]", nbins);
  EBOS_REQUIRE(b >= 1 && b <= 65535 && n >= 0 && H > 0 && W > 0 && row_stride > 0,
               "ebos_warp_voxel: bad sizes b=%lld n=%lld H=%d W=%d stride=%d", (long long)b, (long long)n, H, W, row_stride);
  if (n == 0) return EBOS_OK;
  dim3 grid(stream_grid(n, 256), (unsigned)b);
  warp_voxel_kernel<T><<<grid, dim3(256), 0, as_stream(stream)>>>(events, voxel, tminmax, ref_mode, ref_fraction, normalize_t, n,
                                                                  nbins, H, W, row_stride, bins, warped, oob_count);
  EBOS_CHECK_LAUNCH("ebos_warp_voxel");
  return EBOS_OK;
}

template <typename T>
int warp_voxel_bwd_impl(const T* events, const T* tminmax, int ref_mode, double ref_fraction, int normalize_t,
                        const T* d_warped, int64_t b, int64_t n, int nbins, int H, int W, int row_stride,
                        const uint8_t* bins, T* d_voxel, ebos_stream_t stream) {
  EBOS_REQUIRE(tminmax && d_voxel, "ebos_warp_voxel_bwd: NULL tminmax/d_voxel");
  EBOS_REQUIRE((events && d_warped && bins) || n == 0, "ebos_warp_voxel_bwd: NULL events/d_warped/bins");
  EBOS_REQUIRE(ref_mode_ok(ref_mode), "ebos_warp_voxel_bwd: bad ref_mode %d", ref_mode);
  EBOS_REQUIRE(bins_ok(nbins), "ebos_warp_voxel_bwd: T = %d is outside [1, 255]", nbins);
  EBOS_REQUIRE(b >= 1 && b <= 65535 && n >= 0 && H > 0 && W > 0 && row_stride > 0, "ebos_warp_voxel_bwd: bad sizes");
  if (n == 0) return EBOS_OK;
  dim3 grid(stream_grid(n, 256), (unsigned)b);
  warp_voxel_bwd_kernel<T><<<grid, dim3(256), 0, as_stream(stream)>>>(events, tminmax, ref_mode, ref_fraction, normalize_t,
                                                                      d_warped, n, nbins, H, W, row_stride, bins, d_voxel);
  EBOS_CHECK_LAUNCH("ebos_warp_voxel_bwd");
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

int ebos_event_time_bins_f32(const float* events, const float* tminmax, int64_t b, int64_t n, int T, uint8_t* bins,
                             ebos_stream_t stream) {
  return ebos::time_bins_impl<float>(events, tminmax, b, n, T, bins, stream);
}
int ebos_event_time_bins_f64(const double* events, const double* tminmax, int64_t b, int64_t n, int T, uint8_t* bins,
                             ebos_stream_t stream) {
  return ebos::time_bins_impl<double>(events, tminmax, b, n, T, bins, stream);
}

int ebos_warp_voxel_f32(const float* events, const float* voxel, const float* tminmax, int ref_mode, double ref_fraction,
                        int normalize_t, int64_t b, int64_t n, int T, int H, int W, int row_stride, const uint8_t* bins,
                        float* warped, int32_t* oob_count, ebos_stream_t stream) {
  return ebos::warp_voxel_impl<float>(events, voxel, tminmax, ref_mode, ref_fraction, normalize_t, b, n, T, H, W, row_stride,
                                      bins, warped, oob_count, stream);
}
int ebos_warp_voxel_f64(const double* events, const double* voxel, const double* tminmax, int ref_mode, double ref_fraction,
                        int normalize_t, int64_t b, int64_t n, int T, int H, int W, int row_stride, const uint8_t* bins,
                        double* warped, int32_t* oob_count, ebos_stream_t stream) {
  return ebos::warp_voxel_impl<double>(events, voxel, tminmax, ref_mode, ref_fraction, normalize_t, b, n, T, H, W, row_stride,
                                       bins, warped, oob_count, stream);
}
int ebos_warp_voxel_bwd_f32(const float* events, const float* tminmax, int ref_mode, double ref_fraction, int normalize_t,
                            const float* d_warped, int64_t b, int64_t n, int T, int H, int W, int row_stride,
                            const uint8_t* bins, float* d_voxel, ebos_stream_t stream) {
  return ebos::warp_voxel_bwd_impl<float>(events, tminmax, ref_mode, ref_fraction, normalize_t, d_warped, b, n, T, H, W,
                                          row_stride, bins, d_voxel, stream);
}
int ebos_warp_voxel_bwd_f64(const double* events, const double* tminmax, int ref_mode, double ref_fraction, int normalize_t,
                            const double* d_warped, int64_t b, int64_t n, int T, int H, int W, int row_stride,
                            const uint8_t* bins, double* d_voxel, ebos_stream_t stream) {
  return ebos::warp_voxel_bwd_impl<double>(events, tminmax, ref_mode, ref_fraction, normalize_t, d_warped, b, n, T, H, W,
                                           row_stride, bins, d_voxel, stream);
}

int ebos_iwe_voxel_f32(const float* x, const float* y, const float* dt, const float* weight, const uint8_t* bins, int64_t n,
                       const float* voxel, int T, int H, int W, int row_stride, int pad_h, int pad_w, float* iwe,
                       ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(voxel && iwe, "ebos_iwe_voxel: NULL voxel/iwe");
  EBOS_REQUIRE((x && y && dt && bins) || n == 0, "ebos_iwe_voxel: NULL event buffer");
  EBOS_REQUIRE(bins_ok(T), "ebos_iwe_voxel: T = %d is outside [1, 255]", T);
  EBOS_REQUIRE(n >= 0 && H > 0 && W > 0 && row_stride > 0 && pad_h >= 0 && pad_w >= 0, "ebos_iwe_voxel: bad sizes");
  if (n == 0) return EBOS_OK;
  iwe_voxel_kernel<<<dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream)>>>(x, y, dt, weight, bins, n, voxel, T, H, W,
                                                                                   row_stride, pad_h, pad_w, iwe);
  EBOS_CHECK_LAUNCH("ebos_iwe_voxel");
  return EBOS_OK;
}

int ebos_iwe_voxel_tiled_f32(const float* xs, const float* ys, const float* dts, const float* weight, const uint8_t* bins,
                             const int32_t* key_offsets, int64_t n, const float* voxel, int T, int H, int W, int tile_h,
                             int tile_w, int halo, int splits, int pad_h, int pad_w, float* iwe, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(voxel && iwe && key_offsets, "ebos_iwe_voxel_tiled: NULL voxel/iwe/key_offsets");
  EBOS_REQUIRE((xs && ys && dts && bins) || n == 0, "ebos_iwe_voxel_tiled: NULL event buffer");
  EBOS_REQUIRE(bins_ok(T), "ebos_iwe_voxel_tiled: T = %d is outside [1, 255]", T);
  EBOS_REQUIRE(n >= 0 && H > 0 && W > 0 && pad_h >= 0 && pad_w >= 0 && splits >= 1 && splits <= 64,
               "ebos_iwe_voxel_tiled: bad sizes (splits=%d)", splits);
  if (n == 0) return EBOS_OK;
  hipStream_t s = as_stream(stream);
  const int rc = dispatch_tiled(tile_h, tile_w, halo, [&](auto t) {
    return launch_voxel_tiled<t.th, t.tw, t.halo>(xs, ys, dts, weight, bins, key_offsets, voxel, T, H, W, splits, pad_h, pad_w, iwe, s);
  });
  if (rc == EBOS_ERR_UNSUPPORTED) {
    set_error("ebos_iwe_voxel_tiled: no kernel built for tile %dx%d halo %d (see ebos_tiled_config)", tile_h, tile_w, halo);
    return rc;
  }
  if (rc != EBOS_OK) return rc;
  EBOS_CHECK_LAUNCH("ebos_iwe_voxel_tiled");
  return EBOS_OK;
}

int ebos_iwe_voxel_tiled_batch_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                   const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H, int W,
                                   int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w, float* iwe,
                                   ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(B >= 1 && B <= kMaxWindows, "ebos_iwe_voxel_tiled_batch: B = %d is outside [1, %d]", B, kMaxWindows);
  EBOS_REQUIRE(voxel && iwe && key_offsets && ns, "ebos_iwe_voxel_tiled_batch: NULL voxel/iwe/key_offsets/ns");
  EBOS_REQUIRE(bins_ok(T), "ebos_iwe_voxel_tiled_batch: T = %d is outside [1, 255]", T);
  EBOS_REQUIRE(H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && pad_h >= 0 && pad_w >= 0 && splits >= 1 && splits <= 64,
               "ebos_iwe_voxel_tiled_batch: bad sizes (splits=%d)", splits);
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    EBOS_REQUIRE(ns[b] >= 0, "ebos_iwe_voxel_tiled_batch: window %d has n = %lld", b, (long long)ns[b]);
    total += ns[b];
    EBOS_REQUIRE(total <= INT32_MAX, "ebos_iwe_voxel_tiled_batch: more than INT32_MAX events in the batch");
  }
  EBOS_REQUIRE((xs && ys && dts && bins) || total == 0, "ebos_iwe_voxel_tiled_batch: NULL event buffer");
  if (total == 0) return EBOS_OK;
  hipStream_t s = as_stream(stream);
  const int rc = dispatch_tiled(tile_h, tile_w, halo, [&](auto t) {
    return launch_voxel_tiled_batch<t.th, t.tw, t.halo>(xs, ys, dts, bins, key_offsets, B, voxel, T, H, W, splits, pad_h, pad_w, iwe, s);
  });
  if (rc == EBOS_ERR_UNSUPPORTED) {
    // (tile, halo) is no built configuration: the general kernel, window by window (any event order, global float atomics)
    const int64_t cells = (int64_t)T * 2 * H * W, img = (int64_t)(H + 2 * pad_h) * (W + 2 * pad_w);
    int64_t at = 0;
    for (int b = 0; b < B; ++b) {
      if (int r = ebos_iwe_voxel_f32(xs + at, ys + at, dts + at, nullptr, bins + at, ns[b], voxel + b * cells, T, H, W, W, pad_h, pad_w,
                                     iwe + b * img, stream))
        return r;
      at += ns[b];
    }
    return EBOS_OK;
  }
  if (rc != EBOS_OK) return rc;
  EBOS_CHECK_LAUNCH("ebos_iwe_voxel_tiled_batch");
  return EBOS_OK;
}

int ebos_iwe_voxel_bwd_f32(const float* x, const float* y, const float* dt, const float* weight, const uint8_t* bins,
                           int64_t n, const float* voxel, int T, int H, int W, int row_stride, int pad_h, int pad_w,
                           const float* g_image, const float* affine, int g_lo, int sorted, float* d_voxel, float* d_weight,
                           ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(voxel && g_image && d_voxel, "ebos_iwe_voxel_bwd: NULL voxel/g_image/d_voxel");
  EBOS_REQUIRE((x && y && dt && bins) || n == 0, "ebos_iwe_voxel_bwd: NULL event buffer");
  EBOS_REQUIRE(bins_ok(T), "ebos_iwe_voxel_bwd: T = %d is outside [1, 255]", T);
  EBOS_REQUIRE(n >= 0 && H > 0 && W > 0 && row_stride > 0 && pad_h >= 0 && pad_w >= 0 && g_lo >= 0,
               "ebos_iwe_voxel_bwd: bad sizes");
  if (n == 0) return EBOS_OK;
  dim3 grid(stream_grid(n, 256)), block(256);
  hipStream_t s = as_stream(stream);
  if (sorted)
    iwe_voxel_bwd_kernel<true><<<grid, block, 0, s>>>(x, y, dt, weight, bins, n, voxel, T, H, W, row_stride, pad_h, pad_w,
                                                      g_image, affine, g_lo, d_voxel, d_weight);
  else
    iwe_voxel_bwd_kernel<false><<<grid, block, 0, s>>>(x, y, dt, weight, bins, n, voxel, T, H, W, row_stride, pad_h, pad_w,
                                                       g_image, affine, g_lo, d_voxel, d_weight);
  EBOS_CHECK_LAUNCH("ebos_iwe_voxel_bwd");
  return EBOS_OK;
}

int ebos_iwe_voxel_owner_bwd_f32(const float* xs, const float* ys, const float* dts, const float* weight, const uint8_t* bins,
                                 const int32_t* key_offsets, int64_t n, const float* voxel, int T, int H, int W, int tile_h,
                                 int tile_w, int pad_h, int pad_w, const float* g_image, const float* affine, int g_lo,
                                 float* d_voxel, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(voxel && g_image && d_voxel, "ebos_iwe_voxel_owner_bwd: NULL voxel/g_image/d_voxel");
  EBOS_REQUIRE(key_offsets, "ebos_iwe_voxel_owner_bwd: key_offsets is NULL (the kernel needs a binned plan)");
  EBOS_REQUIRE((xs && ys && dts && bins) || n == 0, "ebos_iwe_voxel_owner_bwd: NULL event buffer");
  EBOS_REQUIRE(bins_ok(T), "ebos_iwe_voxel_owner_bwd: T = %d is outside [1, 255]", T);
  EBOS_REQUIRE(n >= 0 && n <= INT32_MAX && H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && pad_h >= 0 && pad_w >= 0 && g_lo >= 0,
               "ebos_iwe_voxel_owner_bwd: bad sizes");
  const int tiles_y = (H + tile_h - 1) / tile_h, tiles_x = (W + tile_w - 1) / tile_w;
  const int64_t n_keys = (int64_t)tiles_y * tiles_x * tile_h * tile_w;
  EBOS_REQUIRE(n_keys < INT32_MAX, "ebos_iwe_voxel_owner_bwd: %lld keys are more than a plan can hold", (long long)n_keys);
  // (n == 0 still runs: every cell is written, with zeros)
  iwe_voxel_owner_bwd_kernel<<<dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(
      xs, ys, dts, weight, bins, key_offsets, (int32_t)n, voxel, T, H, W, tile_h, tile_w, tiles_x, n_keys, pad_h, pad_w, g_image,
      affine, g_lo, d_voxel);
  EBOS_CHECK_LAUNCH("ebos_iwe_voxel_owner_bwd");
  return EBOS_OK;
}

int ebos_iwe_voxel_owner_bwd_batch_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                       const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H, int W,
                                       int tile_h, int tile_w, int pad_h, int pad_w, const float* g_image, const float* affine,
                                       int g_lo, float* d_voxel, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(B >= 1 && B <= kMaxWindows, "ebos_iwe_voxel_owner_bwd_batch: B = %d is outside [1, %d]", B, kMaxWindows);
  EBOS_REQUIRE(voxel && g_image && d_voxel, "ebos_iwe_voxel_owner_bwd_batch: NULL voxel/g_image/d_voxel");
  EBOS_REQUIRE(key_offsets && ns, "ebos_iwe_voxel_owner_bwd_batch: key_offsets / ns is NULL (the kernel needs a stacked binned plan)");
  EBOS_REQUIRE(bins_ok(T), "ebos_iwe_voxel_owner_bwd_batch: T = %d is outside [1, 255]", T);
  EBOS_REQUIRE(H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && pad_h >= 0 && pad_w >= 0 && g_lo >= 0,
               "ebos_iwe_voxel_owner_bwd_batch: bad sizes");
  WindowBases bases{};
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    EBOS_REQUIRE(ns[b] >= 0, "ebos_iwe_voxel_owner_bwd_batch: window %d has n = %lld", b, (long long)ns[b]);
    bases.at[b] = (int32_t)total;
    total += ns[b];
    EBOS_REQUIRE(total <= INT32_MAX, "ebos_iwe_voxel_owner_bwd_batch: more than INT32_MAX events in the batch");
  }
  for (int b = B; b <= kMaxWindows; ++b) bases.at[b] = (int32_t)total;
  EBOS_REQUIRE((xs && ys && dts && bins) || total == 0, "ebos_iwe_voxel_owner_bwd_batch: NULL event buffer");
  const int tiles_y = (H + tile_h - 1) / tile_h, tiles_x = (W + tile_w - 1) / tile_w;
  const int64_t n_keys = (int64_t)tiles_y * tiles_x * tile_h * tile_w;
  EBOS_REQUIRE(n_keys < INT32_MAX, "ebos_iwe_voxel_owner_bwd_batch: %lld keys are more than a plan can hold", (long long)n_keys);
  // (an empty window still runs: every cell of its d_voxel is written, with zeros)
  iwe_voxel_owner_bwd_batch_kernel<<<dim3((unsigned)((n_keys + 255) / 256), (unsigned)B), dim3(256), 0, as_stream(stream)>>>(
      xs, ys, dts, bins, key_offsets, bases, voxel, T, H, W, tile_h, tile_w, tiles_x, n_keys, pad_h, pad_w, g_image, affine, g_lo,
      d_voxel);
  EBOS_CHECK_LAUNCH("ebos_iwe_voxel_owner_bwd_batch");
  return EBOS_OK;
}

}  // extern "C"
