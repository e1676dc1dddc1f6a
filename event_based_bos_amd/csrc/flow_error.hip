// flow_error.hip -- the reference's flow-error metrics (src/utils/flow_utils.py:706-823, calculate_flow_error_tensor / _numpy)
// for a batch of flows in one pass:
//   flow_mask = !isinf(gt_u) & !isinf(gt_v) & |gt_u| > 0 & |gt_v| > 0,  total = flow_mask & event_mask != 0
//   g = gt * total, p = pred * total (a multiplication: NaN / inf anywhere poisons the sums, as in the reference), times
//   time_scale[b] when given;  e = sqrt(dx * dx + dy * dy),  n = count(total) + 1e-5
//   EPE = sum(e) / n,  kPE = count(e > k) / n (k = 1, 2, 3, 5, 10, 20),
//   AE = sum(acos((1 + u u_gt + v v_gt) / (sqrt(1 + u u + v v) sqrt(1 + u_gt u_gt + v_gt v_gt)))) / n
//   and the mean of each over the batch.
//
// The per-pixel arithmetic is the reference's IEEE operations in its order with no contraction (the pragma below; hipcc contracts
// a * b + c into an FMA by default), and sqrt / division are correctly rounded: for float64 flows every pixel's e is bit-equal
// to numpy's, so the threshold counts and n are exact and NaN appears exactly where the reference's does.  float32 flows are
// masked, scaled and differenced in float32 (the reference's elementwise ops); the norm, the AE term and every sum are float64.
//
// Three launches, no atomics, bit-identical from run to run:
//   flow_error_partials  grid (chunk of rows, item): each lane sums e and the AE term in float64 and counts the mask and the six
//                        thresholds; wave shuffles, then LDS across the four waves; one record per workgroup in the caller's slab.
//                        The chunking depends on (H, W) only, so an item gives the same bits alone or in any batch.
//   flow_error_finish    one workgroup per item: its records summed in a fixed order, then the ratios;
//   flow_error_means     one workgroup: the means over the batch.
#pragma clang fp contract(off)

#include "common.h"

namespace ebos {
namespace {

constexpr int kFeBlock = 256;
constexpr int kFeWaves = kFeBlock / kWave;
constexpr int kFePixels = 2048;        // pixels per workgroup (8 per lane): one 720 x 640 item fills 225 workgroups
constexpr int kFeCounts = 7;           // mask, e > 1, 2, 3, 5, 10, 20

struct FePartial {
  double sum_e, sum_ae;
  unsigned long long cnt[kFeCounts];
};

struct FeGeometry {
  int rows, chunks;
};

// The chunking of an item depends on (H, W) alone -- not on B, nor on the device -- so an item's sums are the same bits whether it is
// scored alone or in a batch.
FeGeometry fe_geometry(int H, int W) {
  int64_t c = ((int64_t)H * W + kFePixels - 1) / kFePixels;
  if (c > H) c = H;
  if (c < 1) c = 1;
  FeGeometry g;
  g.rows = (int)((H + c - 1) / c);
  g.chunks = (H + g.rows - 1) / g.rows;
  return g;
}

struct FeArgs {
  const void* gt;
  const void* pred;
  const uint8_t* mask;  // nullable
  const void* ts;       // nullable, [B] of the flow type
  int64_t g_sb, g_sc, g_sr, p_sb, p_sc, p_sr, m_sb, m_sr;
  int H, W, rows, chunks, clamp;
};

struct FeAcc {
  double se, sae;
  unsigned c[kFeCounts];
};

template <typename T>
__device__ __forceinline__ void fe_pixel(T gu, T gv, T pu, T pv, bool ev, bool has_ts, T ts, bool clamp, FeAcc& a) {
  const bool m = ev && !__builtin_isinf(gu) && !__builtin_isinf(gv) && __builtin_fabs(gu) > T(0) && __builtin_fabs(gv) > T(0);
  const T mf = m ? T(1) : T(0);
  T g0 = gu * mf, g1 = gv * mf, p0 = pu * mf, p1 = pv * mf;
  if (has_ts) {
    g0 = g0 * ts;
    g1 = g1 * ts;
    p0 = p0 * ts;
    p1 = p1 * ts;
  }
  const double dx = (double)(g0 - p0), dy = (double)(g1 - p1);
  const double e = __builtin_sqrt(dx * dx + dy * dy);
  const double u = p0, v = p1, ug = g0, vg = g1;
  double cs = ((1.0 + u * ug) + v * vg) / (__builtin_sqrt((1.0 + u * u) + v * v) * __builtin_sqrt((1.0 + ug * ug) + vg * vg));
  if (clamp) cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);  // (NaN stays NaN)
  a.se += e;
  a.sae += acos(cs);
  a.c[0] += m;
  a.c[1] += e > 1.0;
  a.c[2] += e > 2.0;
  a.c[3] += e > 3.0;
  a.c[4] += e > 5.0;
  a.c[5] += e > 10.0;
  a.c[6] += e > 20.0;
}

// V consecutive elements (16 bytes when V > 1; the host checked the alignment)
template <typename T, int V>
struct FeVec {
  T v[V];
};
template <typename T, int V>
__device__ __forceinline__ FeVec<T, V> fe_load(const T* p) {
  FeVec<T, V> r;
  if constexpr (V == 1) {
    r.v[0] = *p;
  } else if constexpr (sizeof(T) == 8) {
    const double2 q = *reinterpret_cast<const double2*>(p);
    r.v[0] = q.x;
    r.v[1] = q.y;
  } else {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r.v[0] = q.x;
    r.v[1] = q.y;
    r.v[2] = q.z;
    r.v[3] = q.w;
  }
  return r;
}
template <int V>
__device__ __forceinline__ unsigned fe_load_mask(const uint8_t* p) {  // byte k of the result = element k
  if constexpr (V == 1) return *p;
  else if constexpr (V == 2) return *reinterpret_cast<const uint16_t*>(p);
  else return *reinterpret_cast<const uint32_t*>(p);
}

template <typename T, int V>
__global__ __launch_bounds__(kFeBlock) void flow_error_partials(FeArgs a, FePartial* __restrict__ part) {
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int r0 = chunk * a.rows;
  const int r1 = min(a.H, r0 + a.rows);
  const T* gt = static_cast<const T*>(a.gt) + b * a.g_sb;
  const T* pr = static_cast<const T*>(a.pred) + b * a.p_sb;
  const uint8_t* mk = a.mask ? a.mask + b * a.m_sb : nullptr;
  const bool has_ts = a.ts != nullptr;
  const T ts = has_ts ? static_cast<const T*>(a.ts)[b] : T(1);
  const bool clamp = a.clamp != 0;
  const unsigned wv = (unsigned)(a.W / V);
  const unsigned items = (unsigned)(r1 - r0) * wv;  // (H * W < 2^31: checked on the host)

  FeAcc acc;
  acc.se = 0.0;
  acc.sae = 0.0;
#pragma unroll
  for (int k = 0; k < kFeCounts; ++k) acc.c[k] = 0;

#pragma unroll 2
  for (unsigned i = threadIdx.x; i < items; i += kFeBlock) {
    const int r = r0 + (int)(i / wv);
    const int c = (int)(i % wv) * V;
    const FeVec<T, V> gu = fe_load<T, V>(gt + r * a.g_sr + c);
    const FeVec<T, V> gv = fe_load<T, V>(gt + a.g_sc + r * a.g_sr + c);
    const FeVec<T, V> pu = fe_load<T, V>(pr + r * a.p_sr + c);
    const FeVec<T, V> pv = fe_load<T, V>(pr + a.p_sc + r * a.p_sr + c);
    const unsigned mb = mk ? fe_load_mask<V>(mk + r * a.m_sr + c) : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < V; ++k) fe_pixel<T>(gu.v[k], gv.v[k], pu.v[k], pv.v[k], ((mb >> (8 * k)) & 0xffu) != 0, has_ts, ts, clamp, acc);
  }

  // wave, then workgroup, in a fixed order
  double se = wave_sum(acc.se), sae = wave_sum(acc.sae);
  unsigned cnt[kFeCounts];
#pragma unroll
  for (int k = 0; k < kFeCounts; ++k) cnt[k] = wave_sum(acc.c[k]);
  __shared__ double s_sum[kFeWaves][2];
  __shared__ unsigned s_cnt[kFeWaves][kFeCounts];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  if (lane == 0) {
    s_sum[wave][0] = se;
    s_sum[wave][1] = sae;
#pragma unroll
    for (int k = 0; k < kFeCounts; ++k) s_cnt[wave][k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    FePartial p;
    p.sum_e = s_sum[0][0];
    p.sum_ae = s_sum[0][1];
#pragma unroll
    for (int k = 0; k < kFeCounts; ++k) p.cnt[k] = s_cnt[0][k];
    for (int w = 1; w < kFeWaves; ++w) {
      p.sum_e += s_sum[w][0];
      p.sum_ae += s_sum[w][1];
#pragma unroll
      for (int k = 0; k < kFeCounts; ++k) p.cnt[k] += s_cnt[w][k];
    }
    part[(size_t)b * a.chunks + chunk] = p;
  }
}

// a workgroup-wide sum in a fixed order (wave shuffles, then the waves in index order); the result is valid in thread 0
template <typename T>
__device__ __forceinline__ T fe_block_sum(T v, T* s_red) {
  v = wave_sum(v);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  __syncthreads();  // (s_red is reused from one call to the next)
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  T t = s_red[0];
  for (int w = 1; w < kFeWaves; ++w) t += s_red[w];
  return t;
}

// out [(B + 1) x 9]: per item EPE, 1PE, 2PE, 3PE, 5PE, 10PE, 20PE, AE, mask count -- one workgroup per item, each thread summing the
// records k = t, t + 256, ... in order, then the workgroup in a fixed order
__global__ __launch_bounds__(kFeBlock) void flow_error_finish(const FePartial* __restrict__ part, int chunks, double* __restrict__ out) {
  __shared__ double s_d[kFeWaves];
  __shared__ unsigned long long s_u[kFeWaves];
  const int b = blockIdx.x;
  const FePartial* p = part + (size_t)b * chunks;
  double se = 0.0, sae = 0.0;
  unsigned long long c[kFeCounts] = {0, 0, 0, 0, 0, 0, 0};
  for (int k = threadIdx.x; k < chunks; k += kFeBlock) {
    se += p[k].sum_e;
    sae += p[k].sum_ae;
#pragma unroll
    for (int j = 0; j < kFeCounts; ++j) c[j] += p[k].cnt[j];
  }
  se = fe_block_sum(se, s_d);
  sae = fe_block_sum(sae, s_d);
#pragma unroll
  for (int j = 0; j < kFeCounts; ++j) c[j] = fe_block_sum(c[j], s_u);
  if (threadIdx.x == 0) {
    const double n = (double)c[0] + 1e-5;
    double* o = out + (size_t)b * 9;
    o[0] = se / n;
#pragma unroll
    for (int j = 1; j < kFeCounts; ++j) o[j] = (double)c[j] / n;
    o[7] = sae / n;
    o[8] = (double)c[0];
  }
}

// out row B = the mean over the batch of each column
__global__ __launch_bounds__(kFeBlock) void flow_error_means(int B, double* __restrict__ out) {
  __shared__ double s_d[kFeWaves];
  for (int j = 0; j < 9; ++j) {
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += kFeBlock) s += out[(size_t)b * 9 + j];
    s = fe_block_sum(s, s_d);
    if (threadIdx.x == 0) out[(size_t)B * 9 + j] = s / (double)B;
  }
}

bool fe_aligned(const void* p, int64_t bytes) { return reinterpret_cast<uintptr_t>(p) % (uintptr_t)bytes == 0; }

template <typename T>
int fe_launch(const FeArgs& a, int B, FePartial* part, double* out, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec = a.W % V == 0 && fe_aligned(a.gt, 16) && fe_aligned(a.pred, 16) && a.g_sb % V == 0 && a.g_sc % V == 0 &&
                   a.g_sr % V == 0 && a.p_sb % V == 0 && a.p_sc % V == 0 && a.p_sr % V == 0 &&
                   (!a.mask || (fe_aligned(a.mask, V) && a.m_sb % V == 0 && a.m_sr % V == 0));
  const dim3 grid(a.chunks, B);
  if (vec) hipLaunchKernelGGL((flow_error_partials<T, V>), grid, dim3(kFeBlock), 0, s, a, part);
  else hipLaunchKernelGGL((flow_error_partials<T, 1>), grid, dim3(kFeBlock), 0, s, a, part);
  EBOS_CHECK_LAUNCH("ebos_flow_error: flow_error_partials");
  hipLaunchKernelGGL(flow_error_finish, dim3(B), dim3(kFeBlock), 0, s, part, a.chunks, out);
  EBOS_CHECK_LAUNCH("ebos_flow_error: flow_error_finish");
  hipLaunchKernelGGL(flow_error_means, dim3(1), dim3(kFeBlock), 0, s, B, out);
  EBOS_CHECK_LAUNCH("ebos_flow_error: flow_error_means");
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

size_t ebos_flow_error_scratch_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const ebos::FeGeometry g = ebos::fe_geometry(H, W);
  return (size_t)B * (size_t)g.chunks * sizeof(ebos::FePartial);
}

int ebos_flow_error(int dtype, int B, int H, int W, const void* flow_gt, int64_t gt_sb, int64_t gt_sc, int64_t gt_sr,
                    const void* flow_pred, int64_t pred_sb, int64_t pred_sc, int64_t pred_sr, const uint8_t* event_mask,
                    int64_t mask_sb, int64_t mask_sr, const void* time_scale, int flags, double* out, void* scratch,
                    size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(dtype == EBOS_FLOW_ERROR_F32 || dtype == EBOS_FLOW_ERROR_F64, "ebos_flow_error: dtype %d is not F32 (0) or F64 (1)", dtype);
  EBOS_REQUIRE(B > 0 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "ebos_flow_error: bad shape B = %d, H = %d, W = %d", B, H, W);
  EBOS_REQUIRE(B <= 65535, "ebos_flow_error: B = %d > 65535", B);
  EBOS_REQUIRE(flow_gt && flow_pred && out && scratch, "ebos_flow_error: NULL buffer");
  EBOS_REQUIRE(gt_sb >= 0 && gt_sc >= 0 && gt_sr >= 0 && pred_sb >= 0 && pred_sc >= 0 && pred_sr >= 0 && mask_sb >= 0 && mask_sr >= 0,
               "ebos_flow_error: negative stride");
  EBOS_REQUIRE((flags & ~EBOS_FLOW_ERROR_CLAMP_AE) == 0, "ebos_flow_error: unknown flag bits 0x%x", flags);
  const size_t need = ebos_flow_error_scratch_bytes(B, H, W);
  if (scratch_bytes < need) {
    set_error("ebos_flow_error: scratch too small (%zu < %zu)", scratch_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  const FeGeometry g = fe_geometry(H, W);
  FeArgs a;
  a.gt = flow_gt;
  a.pred = flow_pred;
  a.mask = event_mask;
  a.ts = time_scale;
  a.g_sb = gt_sb;
  a.g_sc = gt_sc;
  a.g_sr = gt_sr;
  a.p_sb = pred_sb;
  a.p_sc = pred_sc;
  a.p_sr = pred_sr;
  a.m_sb = mask_sb;
  a.m_sr = mask_sr;
  a.H = H;
  a.W = W;
  a.rows = g.rows;
  a.chunks = g.chunks;
  a.clamp = flags & EBOS_FLOW_ERROR_CLAMP_AE;
  FePartial* part = static_cast<FePartial*>(scratch);
  return dtype == EBOS_FLOW_ERROR_F64 ? fe_launch<double>(a, B, part, out, as_stream(stream))
                                      : fe_launch<float>(a, B, part, out, as_stream(stream));
}

}  // extern "C"
