// iwe_multiref_slab.hip -- the multi-reference contrast on the tile-private pipeline (gfx950 / CDNA4): the K-image form of the slab
// forward and a tile-private backward that sums over the references inside the tile.
//
// A plan built with normalised time and reference fraction f holds dt = (t - tmin) / (tmax - tmin) - f; reference k is the scalar
// shift shifts[k] = f - r_k (float32, by value).  Per event dt_k = dt + shifts[k] is ONE rounded float32 add before anything else
// uses it -- the values the loop route keeps as plan.dt + shift_k.
//
//   forward   ebos_iwe_dense_slab_multiref_f32: the accumulate and combine passes of ebos_iwe_dense_slab_f32 (iwe_tile_core.h) with
//             the reference as an OUTER GRID DIMENSION.  Workgroup (work item, k) keeps ONE fixed-point / f64 LDS window of tile +
//             halo, as the single form does, and writes its slab into workspace k; combine workgroup (pixel block, k) overwrites
//             iwes[k] and leaves variance k.  Two launches whatever K is.  Image k has the bits of the single form run on dt + shifts[k].
//   backward  ebos_iwe_dense_tiled_multiref_bwd_f32: one workgroup per tile keeps the two f64 d_flow planes of its tile in LDS and
//             sweeps the references: stage G_k = a_k g_images[k] + c_k of tile + halo, walk the tile's events with dt_k, add.  Every
//             source pixel of the tile has ONE owner thread, which walks the pixel's run (the events of a pixel are contiguous in a
//             binned plan) in plan order: no atomics at all, the same bits on every call.  A run of more than 64 events (a hot pixel)
//             is walked by its owner's whole wavefront, 64 events at a time, with a fixed butterfly sum.  d_flow [2, H, W] is
//             overwritten once, after the last reference, with plain stores (+ addend).  One launch whatever K is.
//
// Scope: the (x, y, dt) format of an emit="full" binned plan, unit weights, a dense flow, splits >= 1, a built (tile, halo).
// EBOS_ERR_UNSUPPORTED before any launch: adaptive work items (splits = 0) and run-time halo windows (halo < 0).  The compact /
// fractional formats, per-event weights and the patch-grid-sampling route have no argument here.
#include "iwe_tiled_launch.h"

namespace ebos {
namespace {

constexpr int kMaxRef = EBOS_MULTIREF_MAX;
static_assert(kMaxRef == 4, "RefScalars::of selects among four values");

struct RefScalars {  // one float per reference, by value in the kernel arguments
  float at[kMaxRef];
  // (a select chain on constant indices: the struct stays in scalar registers, no indexed copy of it in scratch)
  __device__ __forceinline__ float of(int k) const { return k == 0 ? at[0] : k == 1 ? at[1] : k == 2 ? at[2] : at[3]; }
};

// ---- forward ------------------------------------------------------------------------------------
// workspace k = the single form's workspace (slab_layout) at ws + k * ws_stride: slabs, spill image, partials, SpillEpoch word,
// counters -- every section's contract is the single form's, per reference
template <int TH, int TW, int HALO, int MODE>
__global__ void __launch_bounds__(kBlock)
iwe_slab_multiref_accumulate_kernel(EvPtrs ev, const int32_t* __restrict__ key_offsets, const float* __restrict__ flow, int H, int W,
                                    int tiles_x, int splits, int pad_h, int pad_w, char* __restrict__ ws, size_t ws_stride,
                                    size_t off_spill, size_t off_epoch, RefScalars shifts, unsigned epoch) {
  const int k = blockIdx.y;
  char* wk = ws + (size_t)k * ws_stride;
  accumulate_tile<TH, TW, HALO, false, MODE, FMT_XY, false, false, false, false, false, true>(
      ev, key_offsets, flow, H, W, tiles_x, splits, pad_h, pad_w, reinterpret_cast<float*>(wk), reinterpret_cast<float*>(wk + off_spill),
      GridSrc{}, reinterpret_cast<unsigned*>(wk + off_epoch), epoch, 0.0f, nullptr, shifts.of(k));
}

struct CombineRefs {
  char* ws;
  size_t ws_stride, off_spill, off_partials, off_epoch, off_counters;
  float* iwes;        // [K, h, w]
  float* variances;   // [K], nullable
  double* moments;    // [K, 2], nullable
  long long n_pixels;
  int want_var;
};

// One pixel per thread, for image or padding widths that are no multiple of 4: iwe_slab_combine_kernel's sums in its order (tile row,
// tile column, part; then the spill image) for splits >= 1 and built windows -- iwe_tile_core.h has it as a kernel only, and moving its
// body into a function changed that kernel's register count.
template <int TH, int TW, int HALO>
__device__ __forceinline__ void combine1_block(const float* __restrict__ slabs, float* spill, int tiles_y, int tiles_x, int splits, int H, int W,
                                               int pad_h, int pad_w, float* __restrict__ iwe, int g_lo, double* __restrict__ partials,
                                               const unsigned* __restrict__ spill_epoch, unsigned epoch, const FinalizeIn& fin) {
  const bool spill_used = *spill_epoch == epoch;  // (uniform) some workgroup of THIS call's accumulate pass wrote spill taps
  const __amdgpu_buffer_rsrc_t all_slabs = slab_rsrc(slabs, 0xffffffffu);  // (offsets stay below a workspace's slab section: < 4 GiB)
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  const int h = H + 2 * pad_h, w = W + 2 * pad_w;
  const int R = blockIdx.y, C = blockIdx.x * kCombineBlock + threadIdx.x;
  const int r = R - pad_h, c = C - pad_w;  // un-padded coordinates (may lie in the padding ring)
  float v = 0.0f;
  if (C < w) {
    // tiles whose LDS window [t*T - HALO, t*T + T + HALO) contains r (resp. c)
    int ty0 = (r - HALO - TH + 1 >= 0) ? (r - HALO - TH + 1 + TH - 1) / TH : 0;
    int ty1 = (r + HALO >= 0) ? (r + HALO) / TH : -1;
    if (ty1 > tiles_y - 1) ty1 = tiles_y - 1;
    int tx0 = (c - HALO - TW + 1 >= 0) ? (c - HALO - TW + 1 + TW - 1) / TW : 0;
    int tx1 = (c + HALO >= 0) ? (c + HALO) / TW : -1;
    if (tx1 > tiles_x - 1) tx1 = tiles_x - 1;
    for (int ty = ty0; ty <= ty1; ++ty) {
      for (int tx = tx0; tx <= tx1; ++tx) {
        const int rl = r - (ty * TH - HALO), cl = c - (tx * TW - HALO);
        if ((unsigned)rl >= (unsigned)LH || (unsigned)cl >= (unsigned)LW) continue;
        const unsigned s_byte = ((unsigned)((ty * tiles_x + tx) * splits) * (unsigned)(LH * LW) + (unsigned)(rl * LW + cl)) * 4u;
        for (int p = 0; p < splits; ++p) v += slab_load1(all_slabs, s_byte + (unsigned)p * (unsigned)(LH * LW * 4));
      }
    }
    const int64_t gi = (int64_t)R * w + C;
    const float sp = spill_used ? spill[gi] : 0.0f;
    if (sp != 0.0f) {
      v += sp;
      spill[gi] = 0.0f;  // keep the spill image zero between calls
    }
    iwe[gi] = v;
  }
  if (partials != nullptr) {
    const bool in = C < w && R >= g_lo && R < h - g_lo && C >= g_lo && C < w - g_lo;
    double s = in ? (double)v : 0.0, ss = in ? (double)v * (double)v : 0.0;
    __shared__ double red[2 * kCombineBlock / kWave];
    block_sum2(s, ss, red);
    combine_store_partial(partials, (int64_t)blockIdx.y * gridDim.x + blockIdx.x, (int64_t)gridDim.x * gridDim.y, s, ss, fin);
  }
}

template <int TH, int TW, int HALO, bool VEC>
__global__ void __launch_bounds__(kCombineBlock)
iwe_slab_multiref_combine_kernel(CombineRefs c, int tiles_y, int tiles_x, int splits, int H, int W, int pad_h, int pad_w, int g_lo,
                                 unsigned epoch) {
  const int k = blockIdx.z;
  char* wk = c.ws + (size_t)k * c.ws_stride;
  const float* slabs = reinterpret_cast<const float*>(wk);
  float* spill = reinterpret_cast<float*>(wk + c.off_spill);
  double* partials = c.want_var ? reinterpret_cast<double*>(wk + c.off_partials) : nullptr;
  const unsigned* spill_epoch = reinterpret_cast<const unsigned*>(wk + c.off_epoch);
  float* iwe = c.iwes + (int64_t)k * (H + 2 * pad_h) * (W + 2 * pad_w);
  const FinalizeIn fin{c.want_var == 1 ? reinterpret_cast<unsigned*>(wk + c.off_counters) : nullptr,
                       c.variances ? c.variances + k : nullptr, c.moments ? c.moments + 2 * k : nullptr, c.n_pixels};
  if (VEC)
    combine4_block<TH, TW, HALO, false>(slabs, spill, tiles_y, tiles_x, splits, H, W, pad_h, pad_w, iwe, g_lo, partials, nullptr, spill_epoch,
                                        epoch, nullptr, fin);
  else
    combine1_block<TH, TW, HALO>(slabs, spill, tiles_y, tiles_x, splits, H, W, pad_h, pad_w, iwe, g_lo, partials, spill_epoch, epoch, fin);
}

template <int TH, int TW, int HALO>
int launch_multiref_slab_fwd(const EvPtrs& ev, const int32_t* key_offsets, const float* flow, int H, int W, int splits, int pad_h, int pad_w,
                             const RefScalars& shifts, int K, char* ws, float* iwes, int want_var, int omit, float* variances,
                             double* moments, int acc_mode, hipStream_t s) {
  const size_t lds = (size_t)acc_cells<TH, TW, HALO, false>() * sizeof(double);
  static_assert((size_t)acc_cells<TH, TW, HALO, false>() * sizeof(double) + 1024 <= 160 * 1024, "ONE f64 tile + halo per workgroup");
  const SlabLayout L = slab_layout(H, W, TH, TW, HALO, splits, pad_h, pad_w);
  if (L.off_spill >= ((size_t)1 << 32)) {  // the combine pass addresses a workspace's slab section with 32-bit byte offsets
    set_error("ebos_iwe_dense_slab_multiref: %zu bytes of slabs per reference: the slab section must stay below 4 GiB", L.off_spill);
    return EBOS_ERR_UNSUPPORTED;
  }
  auto ka = acc_mode == ACC_F64 ? iwe_slab_multiref_accumulate_kernel<TH, TW, HALO, ACC_F64>
                                : iwe_slab_multiref_accumulate_kernel<TH, TW, HALO, ACC_FX>;
  if (int rc = reserve_lds(ka, lds, "ebos_iwe_dense_slab_multiref")) return rc;
  const unsigned epoch = next_spill_epoch();
  ka<<<dim3((unsigned)L.nblk, (unsigned)K), dim3(kBlock), lds, s>>>(ev, key_offsets, flow, H, W, L.tiles_x, splits, pad_h, pad_w, ws, L.total,
                                                                    L.off_spill, L.off_epoch, shifts, epoch);
  const int lo = omit ? 1 : 0;
  const long long m_valid = (long long)(L.h - 2 * lo > 0 ? L.h - 2 * lo : 0) * (L.w - 2 * lo > 0 ? L.w - 2 * lo : 0);
  const CombineRefs c{ws, L.total, L.off_spill, L.off_partials, L.off_epoch, L.off_counters, iwes, variances, moments, m_valid, want_var};
  if (L.w % 4 == 0 && pad_w % 4 == 0) {  // (the single form's choice: same grid, same partials, same bits)
    const dim3 gb((L.w / 4 + 63) / 64, (L.h + kCombineRows - 1) / kCombineRows, (unsigned)K);
    iwe_slab_multiref_combine_kernel<TH, TW, HALO, true><<<gb, dim3(kCombineBlock), 0, s>>>(c, L.tiles_y, L.tiles_x, splits, H, W, pad_h,
                                                                                           pad_w, lo, epoch);
  } else {
    const dim3 gb((L.w + kCombineBlock - 1) / kCombineBlock, L.h, (unsigned)K);
    iwe_slab_multiref_combine_kernel<TH, TW, HALO, false><<<gb, dim3(kCombineBlock), 0, s>>>(c, L.tiles_y, L.tiles_x, splits, H, W, pad_h,
                                                                                            pad_w, lo, epoch);
  }
  return EBOS_OK;
}

// ---- backward -----------------------------------------------------------------------------------
constexpr int kHotRun = 64;   // a longer run is walked by the owner's whole wavefront
constexpr int kRunChunk = 4;  // events of a run in flight per owner

struct UpstreamK {  // G_k = a * g + c inside [lo, h - lo) x [lo, w - lo), 0 outside (padded coordinates)
  const float* g;
  float a, c;
  int h, w, lo;
  __device__ __forceinline__ float at(int R, int C) const {
    if (R < lo || R >= h - lo || C < lo || C >= w - lo) return 0.0f;
    return a * g[(int64_t)R * w + C] + c;
  }
};

// -dt_k dL/d(x'_k, y'_k) of one event whose flow cell holds (u, v); s_g: the staged window of G_k, cell (0, 0) = un-padded pixel (oy, ox)
template <int LH, int LW>
__device__ __forceinline__ void event_grad(const UpstreamK& G, const float* s_g, int oy, int ox, int pad_h, int pad_w, float ex, float ey,
                                           float dtk, float u, float v, float& gx, float& gy) {
  const int rs = (int)ex, cs = (int)ey;
  const Taps f = warped_taps(rs, cs, (ex - (float)rs) - dtk * u, (ey - (float)cs) - dtk * v);
  const int rl = f.R - oy, cl = f.C - ox;
  float g00, g10, g01, g11;
  if (f.ok && rl >= 0 && rl < LH - 1 && cl >= 0 && cl < LW - 1) {
    const float* p = &s_g[rl * LW + cl];
    g00 = p[0], g10 = p[LW], g01 = p[1], g11 = p[LW + 1];
  } else {  // beyond the staged halo: the upstream image in global memory
    const int R = f.R + pad_h, C = f.C + pad_w;
    g00 = f.ok ? G.at(R, C) : 0.0f;
    g10 = f.ok ? G.at(R + 1, C) : 0.0f;
    g01 = f.ok ? G.at(R, C + 1) : 0.0f;
    g11 = f.ok ? G.at(R + 1, C + 1) : 0.0f;
  }
  const float a = 1.0f - f.fr, b = 1.0f - f.fc;
  const float dx = b * (g10 - g00) + f.fc * (g11 - g01);  // dL/dx'_k
  const float dy = a * (g01 - g00) + f.fr * (g11 - g10);  // dL/dy'_k
  gx = -dtk * dx;
  gy = -dtk * dy;
}

template <int TH, int TW, int HALO>
__global__ void __launch_bounds__(kBlock)
iwe_tiled_multiref_bwd_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ dts,
                              const int32_t* __restrict__ key_offsets, int32_t n, const float* __restrict__ flow, int H, int W,
                              int tiles_x, int pad_h, int pad_w, RefScalars shifts, RefScalars scales, int K,
                              const float* __restrict__ g_images, const float* __restrict__ affine, int g_lo,
                              const double* __restrict__ var_moments, const float* __restrict__ upstream,
                              const float* __restrict__ addend, float* __restrict__ d_flow) {
  constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO, kPix = TH * TW;
  constexpr int kPer = (kPix + kBlock - 1) / kBlock;  // source pixels per owner thread
  constexpr int kStage = (LH * LW + kBlock - 1) / kBlock;  // window cells per thread
  constexpr int kStageBatch = 4;
  extern __shared__ double s_raw[];
  double* s_d = s_raw;                                 // [2][TH * TW] d_flow accumulators, each cell touched by its owner only
  float* s_g = reinterpret_cast<float*>(s_raw + 2 * kPix);  // [LH][LW] upstream window of the current reference
  const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int tr0 = ty * TH, tc0 = tx * TW, oy = tr0 - HALO, ox = tc0 - HALO;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t hw = (int64_t)H * W;
  const int h = H + 2 * pad_h, w = W + 2 * pad_w;
  const int32_t* __restrict__ ko = key_offsets + (int64_t)tile * kPix;

  // this thread's pixels: their runs (a run never leaves the plan's events, whatever the table holds) and their one flow cell
  int32_t beg[kPer], end[kPer];
  float fu[kPer], fv[kPer];
  int64_t lin[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int pit = (int)threadIdx.x + j * kBlock;
    const int rl = pit / TW, cl = pit - rl * TW;
    const int r = tr0 + rl, c = tc0 + cl;
    const bool own = pit < kPix && r < H && c < W;
    lin[j] = own ? (int64_t)r * W + c : -1;
    beg[j] = own ? min(max(ko[pit], 0), n) : 0;
    end[j] = own ? min(max(ko[pit + 1], beg[j]), n) : 0;
    const bool any = end[j] > beg[j];
    fu[j] = any ? flow[lin[j]] : 0.0f;
    fv[j] = any ? flow[hw + lin[j]] : 0.0f;
    if (pit < kPix) s_d[pit] = 0.0, s_d[kPix + pit] = 0.0;
  }
  const int32_t tile_beg = min(max(ko[0], 0), n), tile_end = min(max(ko[kPix], tile_beg), n);

  if (tile_beg < tile_end) {  // (uniform) an empty tile stages and sweeps nothing: its cells are zeros + addend
    for (int k = 0; k < K; ++k) {
      UpstreamK G;
      G.g = g_images + (int64_t)k * h * w;
      G.h = h, G.w = w, G.lo = g_lo;
      if (var_moments != nullptr) {  // g_images are the IWEs; d var_k / d IWE_k = 2 (IWE_k - mean_k) / (M - 1), times upstream, times scales[k]
        const double a = 2.0 * (double)upstream[0] * (double)scales.of(k) / (var_moments[2 * k + 1] - 1.0);
        G.a = (float)a;
        G.c = (float)(-a * var_moments[2 * k]);
      } else {
        G.a = affine ? affine[2 * k] : 1.0f;
        G.c = affine ? affine[2 * k + 1] : 0.0f;
      }
      const float shift = shifts.of(k);
      __syncthreads();  // the previous reference's sweep has read its window
      // (kStageBatch loads of the window in flight at once -- clamped addresses, unconditional --, then their map and LDS stores: a loop
      // of bounds-checked loads is waited for one by one; a whole window at once would not leave the 64 x 64 tiles their registers)
#pragma unroll 1
      for (int q0 = 0; q0 < kStage; q0 += kStageBatch) {
        float raw[kStageBatch];
#pragma unroll
        for (int q = 0; q < kStageBatch; ++q) {
          const int i = min((int)threadIdx.x + (q0 + q) * kBlock, LH * LW - 1);
          const int rl = i / LW, cl = i - rl * LW;
          const int R = min(max(oy + rl + pad_h, 0), h - 1), C = min(max(ox + cl + pad_w, 0), w - 1);
          raw[q] = G.g[(int64_t)R * w + C];
        }
#pragma unroll
        for (int q = 0; q < kStageBatch; ++q) {
          const int i = (int)threadIdx.x + (q0 + q) * kBlock;
          const int rl = i / LW, cl = i - rl * LW;
          const int R = oy + rl + pad_h, C = ox + cl + pad_w;
          const bool valid = R >= g_lo && R < h - g_lo && C >= g_lo && C < w - g_lo;
          if (i < LH * LW) s_g[i] = valid ? G.a * raw[q] + G.c : 0.0f;
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int pit = (int)threadIdx.x + j * kBlock;
        const int len = end[j] - beg[j];
        if (len > 0 && len <= kHotRun) {
          double sx = 0.0, sy = 0.0;
          for (int32_t b0 = beg[j]; b0 < end[j]; b0 += kRunChunk) {
            float ex[kRunChunk], ey[kRunChunk], edt[kRunChunk];
            const int cnt = min(kRunChunk, end[j] - b0);
#pragma unroll
            for (int e = 0; e < kRunChunk; ++e) {
              const int32_t i = b0 + min(e, cnt - 1);  // (clamped: the loads are unconditional, an unused slot repeats the last event)
              ex[e] = xs[i], ey[e] = ys[i], edt[e] = dts[i];
            }
#pragma unroll
            for (int e = 0; e < kRunChunk; ++e) {
              float gx, gy;
              event_grad<LH, LW>(G, s_g, oy, ox, pad_h, pad_w, ex[e], ey[e], __fadd_rn(edt[e], shift), fu[j], fv[j], gx, gy);
              if (e < cnt) sx += (double)gx, sy += (double)gy;
            }
          }
          s_d[pit] += sx;
          s_d[kPix + pit] += sy;
        }
        // the hot pixels of this wave, one after the other, all 64 lanes on each (every value that steers the loops is wave-uniform)
        unsigned long long hot_lanes = __ballot(len > kHotRun);
        while (hot_lanes) {
          const int src = __ffsll((long long)hot_lanes) - 1;
          hot_lanes &= hot_lanes - 1;
          const int32_t hbeg = __shfl(beg[j], src, kWave), hend = __shfl(end[j], src, kWave);
          const float u = __shfl(fu[j], src, kWave), v = __shfl(fv[j], src, kWave);
          double ax = 0.0, ay = 0.0;
          for (int32_t base = hbeg; base < hend; base += kWave) {
            const int32_t i = base + lane;
            float gx = 0.0f, gy = 0.0f;
            if (i < hend) event_grad<LH, LW>(G, s_g, oy, ox, pad_h, pad_w, xs[i], ys[i], __fadd_rn(dts[i], shift), u, v, gx, gy);
            double tx_ = (double)gx, ty_ = (double)gy;
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {  // butterfly: the same tree, and the same total, in every lane
              tx_ += __shfl_xor(tx_, off, kWave);
              ty_ += __shfl_xor(ty_, off, kWave);
            }
            ax += tx_;
            ay += ty_;
          }
          if (lane == src) {
            s_d[pit] += ax;
            s_d[kPix + pit] += ay;
          }
        }
      }
    }
  }
  // every flow pixel belongs to exactly one tile and one owner: consecutive lanes store consecutive columns of an image row
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int pit = (int)threadIdx.x + j * kBlock;
    if (lin[j] >= 0) {
      d_flow[lin[j]] = (float)s_d[pit] + (addend ? addend[lin[j]] : 0.0f);
      d_flow[hw + lin[j]] = (float)s_d[kPix + pit] + (addend ? addend[hw + lin[j]] : 0.0f);
    }
  }
}

template <int TH, int TW, int HALO>
int launch_multiref_tiled_bwd(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int32_t n, const float* flow,
                              int H, int W, int pad_h, int pad_w, const RefScalars& shifts, const RefScalars& scales, int K,
                              const float* g_images, const float* affine, int g_lo, const double* var_moments, const float* upstream,
                              const float* addend, float* d_flow, hipStream_t s) {
  constexpr size_t lds = (size_t)2 * TH * TW * sizeof(double) + (size_t)(TH + 2 * HALO) * (TW + 2 * HALO) * sizeof(float);
  static_assert(lds <= 160 * 1024, "the single backward's LDS budget: two f64 planes of the tile + one f32 window of tile + halo");
  const int tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
  auto kb = iwe_tiled_multiref_bwd_kernel<TH, TW, HALO>;
  if (int rc = reserve_lds(kb, lds, "ebos_iwe_dense_tiled_multiref_bwd")) return rc;
  kb<<<dim3((unsigned)(tiles_y * tiles_x)), dim3(kBlock), lds, s>>>(xs, ys, dts, key_offsets, n, flow, H, W, tiles_x, pad_h, pad_w, shifts,
                                                                    scales, K, g_images, affine, g_lo, var_moments, upstream, addend, d_flow);
  return EBOS_OK;
}

// K, the shifts and the optional per-reference scales (host memory) -> kernel arguments
int read_refs(const char* who, const float* shifts, const float* scales, int K, RefScalars* sh, RefScalars* sc) {
  EBOS_REQUIRE(K >= 1 && K <= kMaxRef, "%s: K = %d is outside [1, %d]", who, K, kMaxRef);
  EBOS_REQUIRE(shifts != nullptr, "%s: shifts is NULL (a host array of K floats)", who);
  for (int k = 0; k < kMaxRef; ++k) sh->at[k] = 0.0f, sc->at[k] = 1.0f;
  for (int k = 0; k < K; ++k) {
    EBOS_REQUIRE(std::isfinite(shifts[k]), "%s: shifts[%d] is not finite", who, k);
    sh->at[k] = shifts[k];
    if (scales != nullptr) {
      EBOS_REQUIRE(std::isfinite(scales[k]), "%s: scales[%d] is not finite", who, k);
      sc->at[k] = scales[k];
    }
  }
  return EBOS_OK;
}

int check_triple(const char* who, int tile_h, int tile_w, int halo, int splits) {
  if (splits == 0) {
    set_error("%s: splits = 0 (adaptive work items) is not built for the multi-reference kernels: pass splits >= 1", who);
    return EBOS_ERR_UNSUPPORTED;
  }
  if (halo < 0) {
    set_error("%s: run-time halo windows (EBOS_HALO_AUTO) are not built for the multi-reference kernels: pass a built halo", who);
    return EBOS_ERR_UNSUPPORTED;
  }
  if (!config_ok(kMultirefSlabConfigs, tile_h, tile_w, halo)) {
    set_error("%s: no kernel built for tile %dx%d halo %d (see ebos_slab_multiref_config)", who, tile_h, tile_w, halo);
    return EBOS_ERR_UNSUPPORTED;
  }
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

int ebos_slab_multiref_config(int* out, int cap) { return ebos::copy_configs(ebos::kMultirefSlabConfigs, out, cap); }

size_t ebos_iwe_slab_multiref_workspace_bytes(int K, int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w) {
  using namespace ebos;
  if (K < 1 || K > kMaxRef || H <= 0 || W <= 0 || splits < 1 || pad_h < 0 || pad_w < 0 || !config_ok(kMultirefSlabConfigs, tile_h, tile_w, halo)) return 0;
  return (size_t)K * slab_layout(H, W, tile_h, tile_w, halo, splits, pad_h, pad_w).total;  // K workspaces of the single form, back to back
}

int ebos_iwe_dense_slab_multiref_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                     const float* flow, int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w,
                                     const float* shifts, int K, void* workspace, size_t workspace_bytes, float* iwes, int want_variance,
                                     int omit_boundary, float* variances, double* moments, ebos_stream_t stream) {
  using namespace ebos;
  const char* who = "ebos_iwe_dense_slab_multiref";
  EBOS_REQUIRE(flow && iwes && key_offsets && workspace, "%s: NULL flow/iwes/key_offsets/workspace", who);
  EBOS_REQUIRE((xs && ys && dts) || n == 0, "%s: NULL event buffer", who);
  RefScalars sh, sc;
  if (int rc = read_refs(who, shifts, nullptr, K, &sh, &sc)) return rc;
  EBOS_REQUIRE(n >= 0 && n <= INT32_MAX && H > 0 && W > 0 && pad_h >= 0 && pad_w >= 0 && splits >= 0 && splits <= 64,
               "%s: bad sizes (splits=%d)", who, splits);
  EBOS_REQUIRE(want_variance >= 0 && want_variance <= 2, "%s: want_variance is 0, 1 or 2", who);
  EBOS_REQUIRE(want_variance != 1 || variances || moments, "%s: variance requested without an output", who);
  if (int rc = check_triple(who, tile_h, tile_w, halo, splits)) return rc;
  const size_t need = ebos_iwe_slab_multiref_workspace_bytes(K, H, W, tile_h, tile_w, halo, splits, pad_h, pad_w);
  if (workspace_bytes < need) {
    set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  const EvPtrs evp{xs, ys, dts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const int rc = dispatch_multiref_slab(tile_h, tile_w, halo, [&](auto t) {
    return launch_multiref_slab_fwd<t.th, t.tw, t.halo>(evp, key_offsets, flow, H, W, splits, pad_h, pad_w, sh, K,
                                                        reinterpret_cast<char*>(workspace), iwes, want_variance, omit_boundary, variances,
                                                        moments, slab_acc_mode(), as_stream(stream));  // (EBOS_SLAB_ACC, as in the single form)
  });
  if (rc != EBOS_OK) return rc;
  EBOS_CHECK_LAUNCH("ebos_iwe_dense_slab_multiref");
  return EBOS_OK;
}

int ebos_iwe_dense_tiled_multiref_bwd_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                          const float* flow, int H, int W, int tile_h, int tile_w, int halo, int pad_h, int pad_w,
                                          const float* shifts, int K, const float* g_images, const float* affine, int g_lo,
                                          const double* var_moments, const float* upstream, const float* scales, const float* addend,
                                          float* d_flow, ebos_stream_t stream) {
  using namespace ebos;
  const char* who = "ebos_iwe_dense_tiled_multiref_bwd";
  EBOS_REQUIRE(flow && g_images && d_flow && key_offsets, "%s: NULL flow/g_images/d_flow/key_offsets", who);
  EBOS_REQUIRE((xs && ys && dts) || n == 0, "%s: NULL event buffer", who);
  EBOS_REQUIRE((var_moments == nullptr) == (upstream == nullptr), "%s: var_moments and upstream come together", who);
  EBOS_REQUIRE(var_moments == nullptr || affine == nullptr, "%s: var_moments (the folded variance gradient) and affine exclude each other", who);
  RefScalars sh, sc;
  if (int rc = read_refs(who, shifts, scales, K, &sh, &sc)) return rc;
  EBOS_REQUIRE(n >= 0 && n <= INT32_MAX && H > 0 && W > 0 && pad_h >= 0 && pad_w >= 0 && g_lo >= 0, "%s: bad sizes", who);
  if (int rc = check_triple(who, tile_h, tile_w, halo, 1)) return rc;
  const int64_t n_keys = (int64_t)((H + tile_h - 1) / tile_h) * ((W + tile_w - 1) / tile_w) * tile_h * tile_w;
  EBOS_REQUIRE(n_keys < INT32_MAX && (int64_t)H * W < INT32_MAX, "%s: a %dx%d image is more than a plan can hold", who, H, W);
  const int rc = dispatch_multiref_slab(tile_h, tile_w, halo, [&](auto t) {
    return launch_multiref_tiled_bwd<t.th, t.tw, t.halo>(xs, ys, dts, key_offsets, (int32_t)n, flow, H, W, pad_h, pad_w, sh, sc, K, g_images,
                                                         affine, g_lo, var_moments, upstream, addend, d_flow, as_stream(stream));
  });
  if (rc != EBOS_OK) return rc;
  EBOS_CHECK_LAUNCH("ebos_iwe_dense_tiled_multiref_bwd");
  return EBOS_OK;
}

}  // extern "C"
