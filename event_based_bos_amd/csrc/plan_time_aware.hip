// plan_time_aware.hip -- the stacked, binned time-aware plans of several windows in one set of launches, straight from the raw
// sensor columns (RawEventStore.load_raw: col int16, row int16, t int32 | int64 ticks).
//
// Window b = events [begin_b, end_b) of the columns (host table; the ranges may overlap, come in any order, be empty).  An event is
// kept when it passes the CROP and removal rectangles (evaluation._keep_mask) and its pixel lies inside the image.  What a window
// holds is what EventPlan.build(PreparedWindows.events(b), ..., emit="full", time_bin=T) holds -- the float64 [n, 4] array is never
// made -- and the windows' streams lie one after the other as TimeAwarePlanStack lays them out:
//   tick range    over the events that pass the rectangles, then / ticks_per_second in float64 (ebos_raw_time_range)
//   dt            raw_to_soa_kernel's expression (event_plan.hip): float64, one rounding to float32
//   bin           time_bins_kernel's expression (warp_voxel.hip) on t = (double)ticks / ticks_per_second
//   x, y          (float)row, (float)col;  key = source_key's tile-major key
// The order of the events of one source pixel is the order their histogram atomics arrived in: unspecified, as in ebos_bin_events_f32.
//
// Passes (the window is grid dimension y of every one; nine launches whatever B is; nothing waits for the host or for another workgroup):
//   1  init            tick ranges and counts
//   2  memset          the histograms (= the rows of key_offsets_local)
//   3  range           per-window tick range: wave reduction, one int64 atomic min / max per wave
//   4  histogram       per (window, key); the value the atomic returns is kept as the event's rank inside its key; tminmax
//   5-7 scan           exclusive scan of every window's histogram (tiles of 4096, the tile totals, the add-back), the windows' kept
//                      counts, and key_offsets_stacked = local + the kept counts of the earlier windows
//   8  scatter         ONE aligned 16-byte record (dt, index, row | col, bin) per event to its final position (event_plan.hip: a random
//                      4-byte store costs a whole sector, so five arrays cost five)
//   9  unpack          the records, streamed, to the SoA streams
#include "common.h"

namespace ebos {
namespace {

constexpr int kMaxWindows = EBOS_CMAX_VOXEL_MAX_BATCH;
constexpr int kBlock = 256;
constexpr int kScanItems = 16;
constexpr int kScanTile = kBlock * kScanItems;
constexpr long long kTickHi = 0x7fffffffffffffffLL, kTickLo = -0x7fffffffffffffffLL - 1;

struct TaWindows {   // by value: 1 KiB of kernel arguments
  int64_t begin[kMaxWindows];
  int32_t len[kMaxWindows];
  int32_t in_base[kMaxWindows];   // events of the earlier ranges: where the window's ranks lie in scratch
};

struct TaGeom {
  int H, W, tile_h, tile_w, tiles_x, n_keys;
  int has_roi, x0, x1, y0, y1;      // CROP: rows [x0, x1), columns [y0, y1)
  int has_rm, rx0, rx1, ry0, ry1;   // removal rectangle
};

struct alignas(16) TaRecord {
  float dt;
  int32_t idx;
  int32_t rc;    // row << 16 | (col & 0xffff)
  int32_t bin;
};

__device__ __forceinline__ bool passes(const TaGeom& g, int r, int c) {
  bool keep = !g.has_roi || (r >= g.x0 && r < g.x1 && c >= g.y0 && c < g.y1);
  if (g.has_rm && r >= g.rx0 && r < g.rx1 && c >= g.ry0 && c < g.ry1) keep = false;
  return keep;
}

// source_key (event_plan.hip) on integer pixels
__device__ __forceinline__ int pixel_key(const TaGeom& g, int r, int c) {
  if (r < 0 || r >= g.H || c < 0 || c >= g.W) return -1;
  const int ty = r / g.tile_h, tx = c / g.tile_w;
  return (ty * g.tiles_x + tx) * (g.tile_h * g.tile_w) + (r - ty * g.tile_h) * g.tile_w + (c - tx * g.tile_w);
}

__device__ __forceinline__ long long load_ticks(const void* t, int t64, int64_t i) {
  return t64 ? (long long)static_cast<const int64_t*>(t)[i] : (long long)static_cast<const int32_t*>(t)[i];
}

// the bin rule of time_bins_kernel (warp_voxel.hip), every operation rounded on its own
__device__ __forceinline__ int time_bin_of(double t, double tmin, double span, int nbins) {
#pragma clang fp contract(off)
  int k = 0;
  if (span > 0.0) {
    const double tau = (t - tmin) / span;
    const double s = tau * (double)nbins;
    if (s >= (double)nbins) k = nbins - 1;
    else if (s > 0.0) k = (int)s;
  }
  return k;
}

__global__ void ta_init_kernel(long long* __restrict__ ticks, int32_t* __restrict__ counts, int B) {
  const int b = threadIdx.x;
  if (b < B) {
    ticks[2 * b] = kTickHi;
    ticks[2 * b + 1] = kTickLo;
    counts[2 * b] = 0;
    counts[2 * b + 1] = 0;
  }
}

__global__ void __launch_bounds__(kBlock)
ta_range_kernel(const int16_t* __restrict__ col, const int16_t* __restrict__ row, const void* __restrict__ t, int t64, TaWindows w,
                TaGeom g, long long* __restrict__ ticks) {
  const int b = blockIdx.y;
  const int64_t begin = w.begin[b];
  const int len = w.len[b];
  if ((int64_t)blockIdx.x * kBlock >= len) return;   // (uniform over the workgroup)
  long long lo = kTickHi, hi = kTickLo;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < len; i += (int64_t)gridDim.x * kBlock) {
    if (!passes(g, row[begin + i], col[begin + i])) continue;
    const long long v = load_ticks(t, t64, begin + i);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((threadIdx.x & (kWave - 1)) == 0 && lo <= hi) {
    __hip_atomic_fetch_min(&ticks[2 * b], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&ticks[2 * b + 1], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(kBlock)
ta_hist_kernel(const int16_t* __restrict__ col, const int16_t* __restrict__ row, TaWindows w, TaGeom g, int64_t key_stride,
               const long long* __restrict__ ticks, double ticks_per_second, int32_t* hist, int32_t* __restrict__ rank,
               int32_t* counts, double* __restrict__ tminmax) {
  const int b = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // (the range pass is complete: stream order)
    const long long lo = ticks[2 * b], hi = ticks[2 * b + 1];
    tminmax[2 * b] = lo <= hi ? (double)lo / ticks_per_second : 0.0;   // t / 1e6, src/data_loader/ccs.py:295
    tminmax[2 * b + 1] = lo <= hi ? (double)hi / ticks_per_second : 0.0;
  }
  const int64_t begin = w.begin[b];
  const int len = w.len[b];
  if ((int64_t)blockIdx.x * kBlock >= len) return;
  int32_t* h = hist + (int64_t)b * key_stride;
  int32_t* rk = rank + w.in_base[b];
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < len; i += (int64_t)gridDim.x * kBlock) {
    const int r = row[begin + i], c = col[begin + i];
    int32_t v = -1;
    if (passes(g, r, c)) {
      const int key = pixel_key(g, r, c);
      if (key >= 0) v = atomicAdd(&h[key], 1);
      else ++bad;
    }
    rk[i] = v;
  }
  if (bad) atomicAdd(&counts[2 * b + 1], bad);
}

// exclusive scan of one 4096-item tile of one window's histogram in place; tile total -> block_sums[b, blockIdx.x]
__global__ void __launch_bounds__(kBlock) ta_scan_tiles_kernel(int32_t* data, int64_t key_stride, int n, int32_t* block_sums, int nblk) {
  __shared__ int32_t s_wave[kBlock / kWave];
  int32_t* d = data + (int64_t)blockIdx.y * key_stride;
  const int base = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
  int32_t v[kScanItems];
  int32_t sum = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    v[k] = (base + k < n) ? d[base + k] : 0;
    sum += v[k];
  }
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  int32_t inc = sum;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int32_t o = __shfl_up(inc, off, kWave);
    if (lane >= off) inc += o;
  }
  if (lane == kWave - 1) s_wave[wid] = inc;
  __syncthreads();
  int32_t wave_off = 0;
  for (int k = 0; k < wid; ++k) wave_off += s_wave[k];
  int32_t run = wave_off + inc - sum;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (base + k < n) d[base + k] = run;
    run += v[k];
  }
  if (threadIdx.x == kBlock - 1) block_sums[(int64_t)blockIdx.y * nblk + blockIdx.x] = run;
}

// one workgroup per window: exclusive scan of its tile totals; the window's kept events -> totals[b] and counts[b, 0]
__global__ void __launch_bounds__(kBlock) ta_scan_sums_kernel(int32_t* block_sums, int nblk, int32_t* __restrict__ totals,
                                                              int32_t* __restrict__ counts) {
  __shared__ int32_t s_wave[kBlock / kWave];
  __shared__ int32_t s_carry;
  int32_t* bs = block_sums + (int64_t)blockIdx.x * nblk;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  for (int start = 0; start < nblk; start += kBlock) {
    const int i = start + threadIdx.x;
    const int32_t v = (i < nblk) ? bs[i] : 0;
    int32_t inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int32_t o = __shfl_up(inc, off, kWave);
      if (lane >= off) inc += o;
    }
    if (lane == kWave - 1) s_wave[wid] = inc;
    __syncthreads();
    int32_t wave_off = 0;
    for (int k = 0; k < wid; ++k) wave_off += s_wave[k];
    const int32_t carry = s_carry;
    if (i < nblk) bs[i] = carry + wave_off + inc - v;
    __syncthreads();
    if (threadIdx.x == kBlock - 1) s_carry = carry + wave_off + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    totals[blockIdx.x] = s_carry;
    counts[2 * blockIdx.x] = s_carry;
  }
}

// the kept events of the windows in front of window b (B <= 64 loads of one cache line)
__device__ __forceinline__ int32_t window_base(const int32_t* __restrict__ totals, int b) {
  int32_t base = 0;
  for (int k = 0; k < b; ++k) base += totals[k];
  return base;
}

__global__ void __launch_bounds__(kBlock) ta_scan_add_kernel(int32_t* local, int32_t* __restrict__ stacked, int64_t key_stride, int n,
                                                             const int32_t* __restrict__ block_sums, int nblk,
                                                             const int32_t* __restrict__ totals) {
  const int b = blockIdx.y;
  const int32_t off = block_sums[(int64_t)b * nblk + blockIdx.x];
  const int32_t base = window_base(totals, b);
  int32_t* d = local + (int64_t)b * key_stride;
  int32_t* s = stacked + (int64_t)b * key_stride;
  const int first = blockIdx.x * kScanTile;
  for (int k = threadIdx.x; k < kScanTile; k += kBlock)
    if (first + k < n) {
      const int32_t v = d[first + k] + off;
      d[first + k] = v;
      s[first + k] = v + base;
    }
}

__global__ void __launch_bounds__(kBlock)
ta_scatter_kernel(const int16_t* __restrict__ col, const int16_t* __restrict__ row, const void* __restrict__ t, int t64, TaWindows w,
                  TaGeom g, int64_t key_stride, const long long* __restrict__ ticks, double ticks_per_second, int ref_mode,
                  double ref_fraction, int normalize_t, int nbins, const int32_t* __restrict__ local, const int32_t* __restrict__ rank,
                  const int32_t* __restrict__ totals, TaRecord* __restrict__ rec) {
  const int b = blockIdx.y;
  const int64_t begin = w.begin[b];
  const int len = w.len[b];
  if ((int64_t)blockIdx.x * kBlock >= len) return;
  // the time base of raw_to_soa_kernel (event_plan.hip)
  const double tmin = (double)ticks[2 * b] / ticks_per_second, tmax = (double)ticks[2 * b + 1] / ticks_per_second;
  double ref;
  if (ref_mode == EBOS_REF_FIRST) ref = tmin;
  else if (ref_mode == EBOS_REF_LAST) ref = tmax;
  else ref = tmin + (tmax - tmin) * ref_fraction;
  const double inv_period = normalize_t ? 1.0 / (tmax - tmin) : 1.0;
  const double span = tmax - tmin;
  const int32_t* off = local + (int64_t)b * key_stride;
  const int32_t* rk = rank + w.in_base[b];
  TaRecord* out = rec + window_base(totals, b);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < len; i += (int64_t)gridDim.x * kBlock) {
    const int32_t rnk = rk[i];
    if (rnk < 0) continue;
    const int r = row[begin + i], c = col[begin + i];
    const int key = pixel_key(g, r, c);   // (>= 0: the histogram pass ranked the event)
    const double ts = (double)load_ticks(t, t64, begin + i) / ticks_per_second;
    TaRecord v;
    v.dt = (float)((ts - ref) * inv_period);
    v.idx = (int32_t)i;
    v.rc = (int32_t)(((uint32_t)r << 16) | ((uint32_t)c & 0xffffu));
    v.bin = time_bin_of(ts, tmin, span, nbins);
    out[off[key] + rnk] = v;   // one 16-byte store
  }
}

__global__ void __launch_bounds__(kBlock)
ta_unpack_kernel(const TaRecord* __restrict__ rec, const int32_t* __restrict__ totals, float* __restrict__ xs, float* __restrict__ ys,
                 float* __restrict__ dts, uint8_t* __restrict__ bins, int32_t* __restrict__ perm) {
  const int b = blockIdx.y;
  const int32_t n = totals[b];
  if ((int64_t)blockIdx.x * kBlock >= n) return;
  const int64_t base = window_base(totals, b);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const TaRecord v = rec[base + i];
    xs[base + i] = (float)(v.rc >> 16);             // x = row
    ys[base + i] = (float)(int16_t)(v.rc & 0xffff);   // y = column
    dts[base + i] = v.dt;
    bins[base + i] = (uint8_t)v.bin;
    perm[base + i] = v.idx;
  }
}

inline size_t ta_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct TaScratch {
  size_t ticks, totals, block_sums, rank, records, bytes;
  int nblk;
};

// false: bad geometry / ranges
bool ta_scratch_layout(const int64_t* ranges, int B, int H, int W, int tile_h, int tile_w, TaScratch* L, int64_t* total_len) {
  if (ranges == nullptr || B < 1 || B > kMaxWindows || H <= 0 || W <= 0 || tile_h <= 0 || tile_w <= 0) return false;
  const int64_t tiles = (int64_t)((H + tile_h - 1) / tile_h) * ((W + tile_w - 1) / tile_w);
  const int64_t n_keys = tiles * tile_h * tile_w;
  if (n_keys + 1 > 0x7fffffffLL) return false;
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = ranges[2 * b + 1] - ranges[2 * b];
    if (ranges[2 * b] < 0 || n < 0) return false;
    total += n;
    if (total > 0x7fffffffLL) return false;
  }
  L->nblk = (int)((n_keys + 1 + kScanTile - 1) / kScanTile);
  size_t at = 0;
  L->ticks = at, at += ta_align((size_t)B * 2 * sizeof(long long));
  L->totals = at, at += ta_align((size_t)B * sizeof(int32_t));
  L->block_sums = at, at += ta_align((size_t)B * L->nblk * sizeof(int32_t));
  L->rank = at, at += ta_align((size_t)total * sizeof(int32_t));
  L->records = at, at += ta_align((size_t)total * sizeof(TaRecord));
  L->bytes = at + 256;
  *total_len = total;
  return true;
}

}  // namespace
}  // namespace ebos

extern "C" {

size_t ebos_plan_time_aware_batch_scratch_bytes(const int64_t* ranges, int B, int H, int W, int tile_h, int tile_w) {
  using namespace ebos;
  TaScratch L;
  int64_t total;
  return ta_scratch_layout(ranges, B, H, W, tile_h, tile_w, &L, &total) ? L.bytes : 0;
}

int ebos_plan_time_aware_raw_batch(const int16_t* col, const int16_t* row, const void* t, int t_is_64, double ticks_per_second,
                                   int64_t n_total, const int64_t* ranges, int B, int has_roi, int xmin, int xmax, int ymin, int ymax,
                                   int has_remove, int rm_x0, int rm_x1, int rm_y0, int rm_y1, int ref_mode, double ref_fraction,
                                   int normalize_t, int T, int H, int W, int tile_h, int tile_w, float* xs, float* ys, float* dts,
                                   uint8_t* bins, int32_t* perm, int64_t capacity, int32_t* key_offsets_local,
                                   int32_t* key_offsets_stacked, int64_t key_stride, int32_t* counts, double* tminmax, void* scratch,
                                   size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  const char* who = "ebos_plan_time_aware_raw_batch";
  EBOS_REQUIRE(B >= 1 && B <= kMaxWindows, "%s: B = %d is outside [1, %d]", who, B, kMaxWindows);
  EBOS_REQUIRE(T >= 1 && T <= 255, "%s: T = %d is outside [1, 255]", who, T);
  EBOS_REQUIRE(H > 0 && W > 0 && tile_h > 0 && tile_w > 0 && H <= 32767 && W <= 32767, "%s: bad sizes %d x %d, tile %d x %d", who, H, W,
               tile_h, tile_w);
  EBOS_REQUIRE(ref_mode >= 0 && ref_mode <= 2, "%s: ref_mode must be FIRST / LAST / FRACTION", who);
  EBOS_REQUIRE(ticks_per_second > 0.0 && n_total >= 0, "%s: ticks_per_second must be > 0, n_total >= 0", who);
  EBOS_REQUIRE(ranges != nullptr, "%s: ranges is NULL", who);
  EBOS_REQUIRE((col && row && t) || n_total == 0, "%s: NULL raw column", who);
  EBOS_REQUIRE(xs && ys && dts && bins && perm && key_offsets_local && key_offsets_stacked && counts && tminmax && scratch,
               "%s: NULL output / scratch", who);
  EBOS_REQUIRE(!has_roi || (xmin <= xmax && ymin <= ymax), "%s: bad CROP rectangle", who);
  EBOS_REQUIRE(!has_remove || (rm_x0 <= rm_x1 && rm_y0 <= rm_y1), "%s: bad removal rectangle", who);
  for (int b = 0; b < B; ++b)
    EBOS_REQUIRE(ranges[2 * b] >= 0 && ranges[2 * b + 1] >= ranges[2 * b] && ranges[2 * b + 1] <= n_total,
                 "%s: window %d = [%lld, %lld) outside the %lld events", who, b, (long long)ranges[2 * b], (long long)ranges[2 * b + 1],
                 (long long)n_total);
  TaScratch L;
  int64_t total = 0;
  EBOS_REQUIRE(ta_scratch_layout(ranges, B, H, W, tile_h, tile_w, &L, &total), "%s: more than INT32_MAX events or keys", who);
  EBOS_REQUIRE(capacity >= total, "%s: capacity %lld < the %lld events of the ranges", who, (long long)capacity, (long long)total);
  TaGeom g;
  g.H = H, g.W = W, g.tile_h = tile_h, g.tile_w = tile_w;
  g.tiles_x = (W + tile_w - 1) / tile_w;
  g.n_keys = ((H + tile_h - 1) / tile_h) * g.tiles_x * tile_h * tile_w;
  g.has_roi = has_roi != 0, g.x0 = xmin, g.x1 = xmax, g.y0 = ymin, g.y1 = ymax;
  g.has_rm = has_remove != 0, g.rx0 = rm_x0, g.rx1 = rm_x1, g.ry0 = rm_y0, g.ry1 = rm_y1;
  EBOS_REQUIRE(key_stride >= (int64_t)g.n_keys + 1, "%s: key_stride %lld shorter than a window's %d offsets", who, (long long)key_stride,
               g.n_keys + 1);
  if (scratch_bytes < L.bytes) {
    set_error("%s: scratch too small (%zu < %zu)", who, scratch_bytes, L.bytes);
    return EBOS_ERR_SCRATCH;
  }
  TaWindows w;
  int64_t at = 0, max_len = 0;
  for (int b = 0; b < kMaxWindows; ++b) {
    const int64_t n = b < B ? ranges[2 * b + 1] - ranges[2 * b] : 0;
    w.begin[b] = b < B ? ranges[2 * b] : 0;
    w.len[b] = (int32_t)n;
    w.in_base[b] = (int32_t)at;
    at += n;
    max_len = n > max_len ? n : max_len;
  }
  hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(scratch);
  base += (256 - reinterpret_cast<uintptr_t>(base) % 256) % 256;   // (the 256 spare bytes of the layout)
  long long* ticks = reinterpret_cast<long long*>(base + L.ticks);
  int32_t* totals = reinterpret_cast<int32_t*>(base + L.totals);
  int32_t* block_sums = reinterpret_cast<int32_t*>(base + L.block_sums);
  int32_t* rank = reinterpret_cast<int32_t*>(base + L.rank);
  TaRecord* rec = reinterpret_cast<TaRecord*>(base + L.records);
  const int n_items = g.n_keys + 1;

  ta_init_kernel<<<dim3(1), dim3(kMaxWindows), 0, s>>>(ticks, counts, B);
  if (hipMemsetAsync(key_offsets_local, 0, (size_t)B * key_stride * sizeof(int32_t), s) != hipSuccess) {
    set_error("%s: hipMemsetAsync failed", who);
    return EBOS_ERR_LAUNCH;
  }
  const dim3 ev_grid(stream_grid(max_len, kBlock, 1024), B);
  ta_range_kernel<<<ev_grid, dim3(kBlock), 0, s>>>(col, row, t, t_is_64 != 0, w, g, ticks);
  ta_hist_kernel<<<ev_grid, dim3(kBlock), 0, s>>>(col, row, w, g, key_stride, ticks, ticks_per_second, key_offsets_local, rank, counts,
                                                  tminmax);
  ta_scan_tiles_kernel<<<dim3(L.nblk, B), dim3(kBlock), 0, s>>>(key_offsets_local, key_stride, n_items, block_sums, L.nblk);
  ta_scan_sums_kernel<<<dim3(B), dim3(kBlock), 0, s>>>(block_sums, L.nblk, totals, counts);
  ta_scan_add_kernel<<<dim3(L.nblk, B), dim3(kBlock), 0, s>>>(key_offsets_local, key_offsets_stacked, key_stride, n_items, block_sums,
                                                              L.nblk, totals);
  ta_scatter_kernel<<<ev_grid, dim3(kBlock), 0, s>>>(col, row, t, t_is_64 != 0, w, g, key_stride, ticks, ticks_per_second, ref_mode,
                                                     ref_fraction, normalize_t, T, key_offsets_local, rank, totals, rec);
  ta_unpack_kernel<<<ev_grid, dim3(kBlock), 0, s>>>(rec, totals, xs, ys, dts, bins, perm);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

}  // extern "C"
