// event_filters.hip -- the reference's event filters (src/utils/event_filters.py) on the GPU, bit-identical to its per-event
// Python loops:
//   BAF  continuous_background_activity_filter (:46-97)   ebos_baf_mask
//   HOT  hot_pixel_filter                       (:100-128) ebos_hot_mask
//   and the order-preserving compaction that turns a keep mask back into a window of the same format (ebos_filter_compact).
//
// BAF in parallel.  The reference walks the events in array order with a time map M: M[x, y] = max(M[x, y], t), then keeps the
// event iff t - (the (s+1)-th largest value of M over the clipped (2k+1)^2 neighbourhood) < dt.  When event i is looked at, M at a
// pixel q is M0[q] maxed with the times of q's events of index <= i.  So:
//   1. the events are grouped by pixel with event index ascending inside each group: a stable LSD radix sort of the pixel keys
//      (8-bit digits; each pass = per-workgroup digit histograms, the device-wide int32 scan of event_plan.hip, a stable scatter
//      whose ranks come from ballots -- no atomic decides a position, so the grouping is the same on every run whatever the
//      arrival order, and a stuck pixel's run of tens of thousands of events is spread over all workgroups like any other);
//   2. per-pixel run offsets by binary search of the sorted keys;
//   3. the inclusive prefix max of t inside every run: a plain scan of (key, t) pairs under the lexicographic max -- keys do not
//      decrease along the sorted array, so the pair maximum up to a slot carries the maximum time of that slot's own run;
//   4. one thread per event, in sorted order (neighbouring lanes search neighbouring runs): for each neighbour pixel the last slot
//      of its run with event index <= i (binary search), its prefix max against M0, into a top-(s+1) list in registers;
//   5. the final map: the last prefix max of every run against M0.
// Every time is a float64; no floating-point atomic touches any value a BAF decision depends on.
#include "common.h"

namespace ebos {
namespace {

constexpr int kFiltBlock = 256;
constexpr int kSortItems = 16;
constexpr int kSortTile = kFiltBlock * kSortItems;  // events per workgroup of a radix pass / of the prefix-max scan
constexpr int kRadix = 256;                           // 8-bit digits
constexpr int kMinEvents = 10;                        // EventFilter.process: fewer events -> the filter is skipped (:184-187)

struct Source {
  int kind;  // EBOS_FILTER_SRC_*
  int ix, iy, it;
  const void* events;
  const int16_t* col;
  const int16_t* row;
  const void* t;
  const uint8_t* pol;
  double tps;
  int H, W;
};

Source make_source(const ebos_event_source* s, int H, int W) {
  Source o;
  o.kind = s->kind;
  o.ix = s->layout & 3;
  o.iy = (s->layout >> 2) & 3;
  o.it = (s->layout >> 4) & 3;
  o.events = s->events;
  o.col = s->col;
  o.row = s->row;
  o.t = s->t;
  o.pol = s->pol;
  o.tps = s->ticks_per_second;
  o.H = H;
  o.W = W;
  return o;
}

// row, column and time (seconds, float64) of event i; false when its pixel lies outside the sensor.  Pixels are int(x), int(y)
// of the input's own dtype (truncation toward zero: (-1, 0) is pixel 0, like Python's int()); raw ticks / ticks_per_second
// like RawEventStore.load_event (data_loader.py: event row = sensor y, column = sensor x).
__device__ __forceinline__ bool load_event(const Source& s, int64_t i, int& r, int& c, double& t) {
  double x, y;
  if (s.kind == EBOS_FILTER_SRC_F32) {
    const float* e = static_cast<const float*>(s.events) + 4 * i;
    x = e[s.ix];
    y = e[s.iy];
    t = e[s.it];
  } else if (s.kind == EBOS_FILTER_SRC_F64) {
    const double* e = static_cast<const double*>(s.events) + 4 * i;
    x = e[s.ix];
    y = e[s.iy];
    t = e[s.it];
  } else {
    r = s.row[i];
    c = s.col[i];
    const double ticks = s.kind == EBOS_FILTER_SRC_RAW32 ? (double)static_cast<const int32_t*>(s.t)[i]
                                                         : (double)static_cast<const int64_t*>(s.t)[i];
    t = ticks / s.tps;
    return r >= 0 && r < s.H && c >= 0 && c < s.W;
  }
  if (!(x > -1.0 && x < (double)s.H && y > -1.0 && y < (double)s.W)) {  // (NaN too)
    r = c = -1;
    return false;
  }
  r = (int)x;
  c = (int)y;
  return true;
}

__device__ __forceinline__ bool skip_filter(const int32_t* n_in) { return n_in != nullptr && *n_in < kMinEvents; }

// ---------------------------------------------------------------------------------------------- grouping
__global__ void __launch_bounds__(kFiltBlock)
baf_keys_kernel(Source s, int64_t n, const uint8_t* __restrict__ mask_in, const int32_t* n_in, uint32_t* __restrict__ keys,
                int32_t* __restrict__ vals, double* __restrict__ times, int32_t* status) {
  if (skip_filter(n_in)) return;
  const uint32_t P = (uint32_t)s.H * (uint32_t)s.W;
  int bad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int r, c;
    double t;
    const bool ok = load_event(s, i, r, c, t);
    const bool in = mask_in == nullptr || mask_in[i] != 0;
    bad += in && !ok;
    keys[i] = (in && ok) ? (uint32_t)r * (uint32_t)s.W + (uint32_t)c : P;  // (P: not in the filter's input, sorts last)
    vals[i] = (int32_t)i;
    times[i] = t;
  }
  if (bad) atomicAdd(status + EBOS_FILTER_STATUS_OUT_OF_SENSOR, bad);
}

__global__ void __launch_bounds__(kFiltBlock)
radix_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift, int nblk, const int32_t* n_in, int32_t* __restrict__ hist) {
  if (skip_filter(n_in)) return;
  __shared__ int32_t h[kRadix];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSortTile;
#pragma unroll 4
  for (int k = 0; k < kSortItems; ++k) {
    const int64_t j = base + k * kFiltBlock + threadIdx.x;
    if (j < n) atomicAdd(&h[(keys[j] >> shift) & (kRadix - 1)], 1);
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];  // digit-major: the scan gives every (digit, block) its base
}

// stable scatter of one 8-bit digit: items are taken in index order, 256 per round; a lane's rank among the lanes of its wave
// with the same digit comes from eight ballots, the waves before it add their counts through LDS, the rounds before through `run`
__global__ void __launch_bounds__(kFiltBlock)
radix_scatter_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n, int shift, int nblk,
                     const int32_t* n_in, const int32_t* __restrict__ hist, uint32_t* __restrict__ keys_out,
                     int32_t* __restrict__ vals_out) {
  if (skip_filter(n_in)) return;
  constexpr int kWaves = kFiltBlock / kWave;
  __shared__ int32_t run[kRadix];
  __shared__ int32_t cnt[kWaves][kRadix];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  run[tid] = hist[(int64_t)tid * nblk + blockIdx.x];
#pragma unroll
  for (int w = 0; w < kWaves; ++w) cnt[w][tid] = 0;
  __syncthreads();
  const uint64_t lt = (1ull << lane) - 1ull;
  const int64_t base = (int64_t)blockIdx.x * kSortTile;
  for (int k = 0; k < kSortItems; ++k) {
    const int64_t j = base + k * kFiltBlock + tid;
    const bool valid = j < n;
    const uint32_t key = valid ? keys[j] : 0u;
    const int32_t v = valid ? vals[j] : 0;
    const int d = (key >> shift) & (kRadix - 1);
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const uint64_t bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const int rank = __popcll(peers & lt);
    if (valid && (peers >> lane) == 1ull) cnt[wid][d] = __popcll(peers);  // the highest lane of the digit's peers
    __syncthreads();
    if (valid) {
      int pos = run[d] + rank;
      for (int w = 0; w < wid; ++w) pos += cnt[w][d];
      keys_out[pos] = key;
      vals_out[pos] = v;
    }
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      add += cnt[w][tid];
      cnt[w][tid] = 0;
    }
    run[tid] += add;
    __syncthreads();
  }
}

// off[p] = first sorted slot whose key is >= p, p in [0, P]
__global__ void __launch_bounds__(kFiltBlock)
run_offsets_kernel(const uint32_t* __restrict__ sk, int64_t n, uint32_t P, const int32_t* n_in, int32_t* __restrict__ off) {
  if (skip_filter(n_in)) return;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p <= (int64_t)P; p += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sk[mid] < (uint32_t)p) lo = mid + 1;
      else hi = mid;
    }
    off[p] = (int32_t)lo;
  }
}

// ---------------------------------------------------------------------------------------------- per-run prefix max of t
struct KT {
  uint32_t k;
  double t;
};
__device__ __forceinline__ KT kt_max(KT a, KT b) { return (b.k > a.k || (b.k == a.k && b.t > a.t)) ? b : a; }
__device__ __forceinline__ KT kt_identity() { return KT{0u, -__builtin_inf()}; }
__device__ __forceinline__ KT kt_shfl_up(KT v, int off) {
  KT o;
  o.k = __shfl_up(v.k, off, kWave);
  o.t = __shfl_up(v.t, off, kWave);
  return o;
}
__device__ __forceinline__ KT kt_shfl_down(KT v, int off) {
  KT o;
  o.k = __shfl_down(v.k, off, kWave);
  o.t = __shfl_down(v.t, off, kWave);
  return o;
}

__global__ void __launch_bounds__(kFiltBlock)
prefix_aggregate_kernel(const uint32_t* __restrict__ sk, const int32_t* __restrict__ si, const double* __restrict__ times, int64_t n,
                        const int32_t* n_in, uint32_t* __restrict__ agg_k, double* __restrict__ agg_t) {
  if (skip_filter(n_in)) return;
  __shared__ KT s_w[kFiltBlock / kWave];
  const int64_t base = (int64_t)blockIdx.x * kSortTile;
  KT a = kt_identity();
  for (int k = 0; k < kSortItems; ++k) {
    const int64_t j = base + k * kFiltBlock + threadIdx.x;
    if (j < n) a = kt_max(a, KT{sk[j], times[si[j]]});
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) a = kt_max(a, kt_shfl_down(a, off));
  if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    KT b = s_w[0];
    for (int w = 1; w < kFiltBlock / kWave; ++w) b = kt_max(b, s_w[w]);
    agg_k[blockIdx.x] = b.k;
    agg_t[blockIdx.x] = b.t;
  }
}

// one workgroup: exclusive scan of the tile aggregates in place (the carry into every tile)
__global__ void __launch_bounds__(kFiltBlock)
prefix_carry_kernel(uint32_t* agg_k, double* agg_t, int nblk, const int32_t* n_in) {
  if (skip_filter(n_in)) return;
  __shared__ KT s_w[kFiltBlock / kWave];
  __shared__ KT s_carry;
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (threadIdx.x == 0) s_carry = kt_identity();
  __syncthreads();
  for (int start = 0; start < nblk; start += kFiltBlock) {
    const int i = start + threadIdx.x;
    const KT v = i < nblk ? KT{agg_k[i], agg_t[i]} : kt_identity();
    KT inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const KT o = kt_shfl_up(inc, off);
      if (lane >= off) inc = kt_max(inc, o);
    }
    KT exc = kt_shfl_up(inc, 1);
    if (lane == 0) exc = kt_identity();
    if (lane == kWave - 1) s_w[wid] = inc;
    __syncthreads();
    KT pre = s_carry;
    for (int w = 0; w < wid; ++w) pre = kt_max(pre, s_w[w]);
    if (i < nblk) {
      const KT e = kt_max(pre, exc);
      agg_k[i] = e.k;
      agg_t[i] = e.t;
    }
    __syncthreads();
    if (threadIdx.x == kFiltBlock - 1) s_carry = kt_max(pre, inc);
    __syncthreads();
  }
}

// pm[j] = max of t over the slots <= j of j's run (every thread owns kSortItems consecutive slots)
__global__ void __launch_bounds__(kFiltBlock)
prefix_max_kernel(const uint32_t* __restrict__ sk, const int32_t* __restrict__ si, const double* __restrict__ times, int64_t n,
                  const int32_t* n_in, const uint32_t* __restrict__ carry_k, const double* __restrict__ carry_t, double* __restrict__ pm) {
  if (skip_filter(n_in)) return;
  __shared__ KT s_w[kFiltBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int64_t base = (int64_t)blockIdx.x * kSortTile + (int64_t)threadIdx.x * kSortItems;
  KT a = kt_identity();
  for (int k = 0; k < kSortItems; ++k)
    if (base + k < n) a = kt_max(a, KT{sk[base + k], times[si[base + k]]});
  KT inc = a;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const KT o = kt_shfl_up(inc, off);
    if (lane >= off) inc = kt_max(inc, o);
  }
  KT exc = kt_shfl_up(inc, 1);
  if (lane == 0) exc = kt_identity();
  if (lane == kWave - 1) s_w[wid] = inc;
  __syncthreads();
  KT run = KT{carry_k[blockIdx.x], carry_t[blockIdx.x]};
  for (int w = 0; w < wid; ++w) run = kt_max(run, s_w[w]);
  run = kt_max(run, exc);
  for (int k = 0; k < kSortItems; ++k) {
    if (base + k < n) {
      run = kt_max(run, KT{sk[base + k], times[si[base + k]]});
      pm[base + k] = run.t;  // (run.k == sk[base + k]: keys do not decrease along the slots)
    }
  }
}

// ---------------------------------------------------------------------------------------------- BAF query / map / pass-through
template <int KMAX>
__global__ void __launch_bounds__(kFiltBlock)
baf_query_kernel(const uint32_t* __restrict__ sk, const int32_t* __restrict__ si, const double* __restrict__ times,
                 const int32_t* __restrict__ off, const double* __restrict__ pm, const double* __restrict__ m0, int64_t n, int H, int W,
                 int ksize, int num_support, double dt, const int32_t* n_in, uint8_t* __restrict__ mask_out, int32_t* n_out,
                 int32_t* status) {
  if (skip_filter(n_in)) return;
  const uint32_t P = (uint32_t)H * (uint32_t)W;
  int kept = 0, clipped = 0;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t p = sk[j];
    if (p >= P) continue;  // (events outside the filter's input: the tail of the sorted keys)
    const int32_t i = si[j];
    const int r = (int)(p / (uint32_t)W), c = (int)(p - (uint32_t)r * (uint32_t)W);
    const double t = times[i];
    double top[KMAX];  // descending: the KMAX largest values seen
#pragma unroll
    for (int q = 0; q < KMAX; ++q) top[q] = -__builtin_inf();
    const int r0 = max(0, r - ksize), r1 = min(H, r + ksize + 1), c0 = max(0, c - ksize), c1 = min(W, c + ksize + 1);
    for (int rr = r0; rr < r1; ++rr) {
      for (int cc = c0; cc < c1; ++cc) {
        const int q = rr * W + cc;
        double v = m0 != nullptr ? m0[q] : 0.0;
        int lo = off[q], hi = off[q + 1];
        if (hi > lo && si[lo] <= i) {  // last slot of the run with event index <= i
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (si[mid] <= i) lo = mid;
            else hi = mid;
          }
          const double u = pm[lo];
          v = u > v ? u : v;
        }
#pragma unroll
        for (int k = KMAX - 1; k > 0; --k) {
          const double lo_v = v < top[k - 1] ? v : top[k - 1];
          top[k] = lo_v > top[k] ? lo_v : top[k];
        }
        top[0] = v > top[0] ? v : top[0];
      }
    }
    bool keep = false;
    if ((r1 - r0) * (c1 - c0) < num_support + 1) {
      ++clipped;  // the reference's time_array[-1 - num_support_event] raises IndexError here
    } else {
      double last = top[0];
#pragma unroll
      for (int k = 1; k < KMAX; ++k)
        if (k == num_support) last = top[k];
      keep = t - last < dt;
    }
    mask_out[i] = keep;
    kept += keep;
  }
  kept = wave_sum(kept);  // (lane 0)
  clipped = wave_sum(clipped);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (kept) atomicAdd(n_out, kept);
    if (clipped) atomicAdd(status + EBOS_FILTER_STATUS_CLIPPED, clipped);
  }
}

__global__ void __launch_bounds__(kFiltBlock)
baf_map_kernel(const int32_t* __restrict__ off, const double* __restrict__ pm, const double* m0, uint32_t P, const int32_t* n_in,
               double* m_out) {
  const bool skip = skip_filter(n_in);
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < (int64_t)P; q += (int64_t)gridDim.x * blockDim.x) {
    double v = m0 != nullptr ? m0[q] : 0.0;
    if (!skip) {
      const int lo = off[q], hi = off[q + 1];
      if (hi > lo) {
        const double u = pm[hi - 1];
        v = u > v ? u : v;
      }
    }
    m_out[q] = v;  // (m_out may be m0: each pixel is read and written by one thread)
  }
}

// a skipped filter (fewer than kMinEvents events in) passes its input mask and count through
__global__ void __launch_bounds__(kFiltBlock)
pass_through_kernel(const uint8_t* __restrict__ mask_in, int64_t n, const int32_t* n_in, uint8_t* __restrict__ mask_out, int32_t* n_out) {
  if (!skip_filter(n_in)) return;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    mask_out[i] = mask_in != nullptr ? mask_in[i] : 1;
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = *n_in;
}

// ---------------------------------------------------------------------------------------------- HOT
__global__ void __launch_bounds__(kFiltBlock)
hot_count_kernel(Source s, int64_t n, const uint8_t* __restrict__ mask_in, const int32_t* n_in, int32_t* __restrict__ cnt,
                 int32_t* status) {
  if (skip_filter(n_in)) return;
  int bad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int r, c;
    double t;
    const bool ok = load_event(s, i, r, c, t);
    const bool in = mask_in == nullptr || mask_in[i] != 0;
    bad += in && !ok;
    if (in && ok && cnt != nullptr) atomicAdd(&cnt[r * s.W + c], 1);  // (integer counts: the same totals in any order)
  }
  if (bad) atomicAdd(status + EBOS_FILTER_STATUS_OUT_OF_SENSOR, bad);
}

__global__ void __launch_bounds__(kFiltBlock)
hot_mask_kernel(Source s, int64_t n, const uint8_t* __restrict__ mask_in, const int32_t* n_in, const int32_t* __restrict__ cnt,
                const double* __restrict__ iwe, double thresh, uint8_t* __restrict__ mask_out, int32_t* n_out) {
  if (skip_filter(n_in)) return;
  int kept = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int r, c;
    double t;
    const bool ok = load_event(s, i, r, c, t);
    const bool in = mask_in == nullptr || mask_in[i] != 0;
    bool keep = false;
    if (in && ok) {
      const int q = r * s.W + c;
      const double v = iwe != nullptr ? iwe[q] : (double)cnt[q];
      keep = !(v > thresh);  // np.where(iwe > hot_pixel): a count equal to the threshold stays
    }
    mask_out[i] = keep;
    kept += keep;
  }
  kept = wave_sum(kept);
  if ((threadIdx.x & (kWave - 1)) == 0 && kept) atomicAdd(n_out, kept);
}

// ---------------------------------------------------------------------------------------------- compaction
__global__ void __launch_bounds__(kFiltBlock) mask_to_i32_kernel(const uint8_t* __restrict__ mask, int64_t n, int32_t* __restrict__ pos) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) pos[i] = mask[i] != 0;
}

__global__ void __launch_bounds__(kFiltBlock)
compact_kernel(Source s, int64_t n, const uint8_t* __restrict__ mask, const int32_t* __restrict__ pos, void* __restrict__ events_out,
               int16_t* __restrict__ col_out, int16_t* __restrict__ row_out, void* __restrict__ t_out, uint8_t* __restrict__ pol_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!mask[i]) continue;
    const int64_t o = pos[i];
    if (s.kind == EBOS_FILTER_SRC_F32) {
      reinterpret_cast<float4*>(events_out)[o] = reinterpret_cast<const float4*>(s.events)[i];
    } else if (s.kind == EBOS_FILTER_SRC_F64) {
      const double2* e = reinterpret_cast<const double2*>(s.events) + 2 * i;
      double2* d = reinterpret_cast<double2*>(events_out) + 2 * o;
      d[0] = e[0];
      d[1] = e[1];
    } else {
      col_out[o] = s.col[i];
      row_out[o] = s.row[i];
      if (s.kind == EBOS_FILTER_SRC_RAW32) static_cast<int32_t*>(t_out)[o] = static_cast<const int32_t*>(s.t)[i];
      else static_cast<int64_t*>(t_out)[o] = static_cast<const int64_t*>(s.t)[i];
      pol_out[o] = s.pol[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------- host side
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct FilterScratch {  // carved out of the caller's scratch, 256-byte aligned sections
  uint32_t *keys_a, *keys_b, *agg_k;
  int32_t *vals_a, *vals_b, *off, *hist, *block_sums, *cnt;
  double *times, *pm, *agg_t;
  size_t bytes;
};

FilterScratch carve(void* base, int64_t n, int H, int W) {
  const int64_t P = (int64_t)H * W, nb = n > 0 ? n : 1;
  const int64_t nblk = (nb + kSortTile - 1) / kSortTile, nhist = kRadix * nblk;
  const int64_t nscan = nhist > nb ? nhist : nb;  // (the compaction scans n flags with the same block sums)
  char* p = static_cast<char*>(base);
  size_t o = 0;
  FilterScratch s;
  auto take = [&](size_t b) {
    char* q = p ? p + o : nullptr;
    o += align256(b);
    return q;
  };
  s.keys_a = reinterpret_cast<uint32_t*>(take(nb * 4));
  s.keys_b = reinterpret_cast<uint32_t*>(take(nb * 4));
  s.vals_a = reinterpret_cast<int32_t*>(take(nb * 4));  // (also the compaction's positions)
  s.vals_b = reinterpret_cast<int32_t*>(take(nb * 4));
  s.times = reinterpret_cast<double*>(take(nb * 8));
  s.pm = reinterpret_cast<double*>(take(nb * 8));
  s.off = reinterpret_cast<int32_t*>(take((P + 1) * 4));  // (also HOT's per-pixel counts)
  s.cnt = s.off;
  s.hist = reinterpret_cast<int32_t*>(take(nhist * 4));
  s.block_sums = reinterpret_cast<int32_t*>(take((scan_blocks(nscan) + 1) * 4));
  s.agg_k = reinterpret_cast<uint32_t*>(take(nblk * 4));
  s.agg_t = reinterpret_cast<double*>(take(nblk * 8));
  s.bytes = o + 256;
  return s;
}

int check_source(const ebos_event_source* src, int H, int W, const char* what) {
  EBOS_REQUIRE(src != nullptr, "%s: source is NULL", what);
  EBOS_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) - 1, "%s: bad sensor size %d x %d", what, H, W);
  EBOS_REQUIRE(src->n >= 0 && src->n < ((int64_t)1 << 31) - 1, "%s: n = %lld outside [0, 2^31 - 1)", what, (long long)src->n);
  EBOS_REQUIRE(src->kind >= EBOS_FILTER_SRC_F32 && src->kind <= EBOS_FILTER_SRC_RAW64, "%s: unknown source kind %d", what, src->kind);
  if (src->kind <= EBOS_FILTER_SRC_F64) {
    const int ix = src->layout & 3, iy = (src->layout >> 2) & 3, it = (src->layout >> 4) & 3;
    EBOS_REQUIRE(src->events != nullptr || src->n == 0, "%s: events is NULL", what);
    EBOS_REQUIRE(ix != iy && ix != it && iy != it && (src->layout >> 6) == 0, "%s: bad column layout %d", what, src->layout);
  } else {
    EBOS_REQUIRE((src->col && src->row && src->t) || src->n == 0, "%s: NULL raw column", what);
    EBOS_REQUIRE(src->ticks_per_second > 0.0, "%s: ticks_per_second must be > 0", what);
  }
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

size_t ebos_event_filter_scratch_bytes(int64_t n, int H, int W) {
  if (n < 0 || H <= 0 || W <= 0) return 0;
  return ebos::carve(nullptr, n, H, W).bytes;
}

int ebos_baf_mask(const ebos_event_source* src, int H, int W, const uint8_t* mask_in, const int32_t* n_in, double dt, int ksize,
                  int num_support_event, const double* time_map_in, double* time_map_out, uint8_t* mask_out, int32_t* n_out,
                  int32_t* status, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  int rc = check_source(src, H, W, "ebos_baf_mask");
  if (rc != EBOS_OK) return rc;
  EBOS_REQUIRE(time_map_out && n_out && status && scratch && (mask_out || src->n == 0), "ebos_baf_mask: NULL buffer");
  if (ksize < 0 || ksize > 7 || num_support_event < 0 || num_support_event > 15) {
    set_error("ebos_baf_mask: BAF_ksize = %d, BAF_num_support_event = %d outside the supported 0 <= ksize <= 7, "
              "0 <= num_support_event <= 15", ksize, num_support_event);
    return EBOS_ERR_UNSUPPORTED;
  }
  const int64_t n = src->n;
  const size_t need = ebos_event_filter_scratch_bytes(n, H, W);
  if (scratch_bytes < need) {
    set_error("ebos_baf_mask: scratch too small (%zu < %zu)", scratch_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  hipStream_t s = as_stream(stream);
  const Source so = make_source(src, H, W);
  const uint32_t P = (uint32_t)H * (uint32_t)W;
  FilterScratch fs = carve(scratch, n, H, W);
  if (hipMemsetAsync(n_out, 0, 4, s) != hipSuccess || (n > 0 && hipMemsetAsync(mask_out, 0, (size_t)n, s) != hipSuccess)) {
    set_error("ebos_baf_mask: hipMemsetAsync failed");
    return EBOS_ERR_LAUNCH;
  }
  if (n > 0) {
    const dim3 blk(kFiltBlock), g(stream_grid(n, kFiltBlock));
    const int nblk = (int)((n + kSortTile - 1) / kSortTile);
    baf_keys_kernel<<<g, blk, 0, s>>>(so, n, mask_in, n_in, fs.keys_a, fs.vals_a, fs.times, status);
    int bits = 1;
    while (bits < 32 && ((uint64_t)1 << bits) <= P) ++bits;  // keys 0 .. P (P = not in the input)
    uint32_t* k_in = fs.keys_a;
    uint32_t* k_out = fs.keys_b;
    int32_t* v_in = fs.vals_a;
    int32_t* v_out = fs.vals_b;
    for (int shift = 0; shift < bits; shift += 8) {
      radix_hist_kernel<<<dim3(nblk), blk, 0, s>>>(k_in, n, shift, nblk, n_in, fs.hist);
      scan_exclusive_i32(fs.hist, (int64_t)kRadix * nblk, fs.block_sums + scan_blocks((int64_t)kRadix * nblk), fs.block_sums, s);
      radix_scatter_kernel<<<dim3(nblk), blk, 0, s>>>(k_in, v_in, n, shift, nblk, n_in, fs.hist, k_out, v_out);
      uint32_t* tk = k_in;
      k_in = k_out;
      k_out = tk;
      int32_t* tv = v_in;
      v_in = v_out;
      v_out = tv;
    }
    run_offsets_kernel<<<dim3(stream_grid((int64_t)P + 1, kFiltBlock)), blk, 0, s>>>(k_in, n, P, n_in, fs.off);
    prefix_aggregate_kernel<<<dim3(nblk), blk, 0, s>>>(k_in, v_in, fs.times, n, n_in, fs.agg_k, fs.agg_t);
    prefix_carry_kernel<<<dim3(1), blk, 0, s>>>(fs.agg_k, fs.agg_t, nblk, n_in);
    prefix_max_kernel<<<dim3(nblk), blk, 0, s>>>(k_in, v_in, fs.times, n, n_in, fs.agg_k, fs.agg_t, fs.pm);
    const int kmax = num_support_event + 1;
#define EBOS_BAF_QUERY(K)                                                                                                        \
  baf_query_kernel<K><<<g, blk, 0, s>>>(k_in, v_in, fs.times, fs.off, fs.pm, time_map_in, n, H, W, ksize, num_support_event, dt, \
                                        n_in, mask_out, n_out, status)
    if (kmax <= 1) EBOS_BAF_QUERY(1);
    else if (kmax <= 2) EBOS_BAF_QUERY(2);
    else if (kmax <= 4) EBOS_BAF_QUERY(4);
    else if (kmax <= 8) EBOS_BAF_QUERY(8);
    else EBOS_BAF_QUERY(16);
#undef EBOS_BAF_QUERY
    pass_through_kernel<<<g, blk, 0, s>>>(mask_in, n, n_in, mask_out, n_out);
    baf_map_kernel<<<dim3(stream_grid(P, kFiltBlock)), blk, 0, s>>>(fs.off, fs.pm, time_map_in, P, n_in, time_map_out);
  } else {
    baf_map_kernel<<<dim3(stream_grid(P, kFiltBlock)), dim3(kFiltBlock), 0, s>>>(fs.off, fs.pm, time_map_in, P, n_out, time_map_out);
  }
  EBOS_CHECK_LAUNCH("ebos_baf_mask");
  return EBOS_OK;
}

int ebos_hot_mask(const ebos_event_source* src, int H, int W, const uint8_t* mask_in, const int32_t* n_in, double thresh,
                  const double* iwe, uint8_t* mask_out, int32_t* n_out, int32_t* status, void* scratch, size_t scratch_bytes,
                  ebos_stream_t stream) {
  using namespace ebos;
  int rc = check_source(src, H, W, "ebos_hot_mask");
  if (rc != EBOS_OK) return rc;
  EBOS_REQUIRE(n_out && status && (scratch || iwe) && (mask_out || src->n == 0), "ebos_hot_mask: NULL buffer");
  const int64_t n = src->n;
  hipStream_t s = as_stream(stream);
  const Source so = make_source(src, H, W);
  const size_t P = (size_t)H * W;
  int32_t* cnt = nullptr;
  if (iwe == nullptr) {
    const size_t need = ebos_event_filter_scratch_bytes(n, H, W);
    if (scratch_bytes < need) {
      set_error("ebos_hot_mask: scratch too small (%zu < %zu)", scratch_bytes, need);
      return EBOS_ERR_SCRATCH;
    }
    cnt = carve(scratch, n, H, W).cnt;
    if (hipMemsetAsync(cnt, 0, P * 4, s) != hipSuccess) {
      set_error("ebos_hot_mask: hipMemsetAsync failed");
      return EBOS_ERR_LAUNCH;
    }
  }
  if (hipMemsetAsync(n_out, 0, 4, s) != hipSuccess) {
    set_error("ebos_hot_mask: hipMemsetAsync failed");
    return EBOS_ERR_LAUNCH;
  }
  if (n > 0) {
    const dim3 blk(kFiltBlock), g(stream_grid(n, kFiltBlock));
    hot_count_kernel<<<g, blk, 0, s>>>(so, n, mask_in, n_in, cnt, status);
    hot_mask_kernel<<<g, blk, 0, s>>>(so, n, mask_in, n_in, cnt, iwe, thresh, mask_out, n_out);
    pass_through_kernel<<<g, blk, 0, s>>>(mask_in, n, n_in, mask_out, n_out);
  }
  EBOS_CHECK_LAUNCH("ebos_hot_mask");
  return EBOS_OK;
}

int ebos_filter_compact(const ebos_event_source* src, const uint8_t* mask, void* events_out, int16_t* col_out, int16_t* row_out,
                        void* t_out, uint8_t* pol_out, int32_t* n_out, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  int rc = check_source(src, 1, 1, "ebos_filter_compact");
  if (rc != EBOS_OK) return rc;
  const int64_t n = src->n;
  EBOS_REQUIRE(n_out && scratch && (mask || n == 0), "ebos_filter_compact: NULL buffer");
  if (src->kind <= EBOS_FILTER_SRC_F64) EBOS_REQUIRE(events_out || n == 0, "ebos_filter_compact: events_out is NULL");
  else EBOS_REQUIRE((col_out && row_out && t_out && src->pol && pol_out) || n == 0, "ebos_filter_compact: NULL raw column");
  const size_t need = ebos_event_filter_scratch_bytes(n, 1, 1);
  if (scratch_bytes < need) {
    set_error("ebos_filter_compact: scratch too small (%zu < %zu)", scratch_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  hipStream_t s = as_stream(stream);
  if (n == 0) {
    if (hipMemsetAsync(n_out, 0, 4, s) != hipSuccess) {
      set_error("ebos_filter_compact: hipMemsetAsync failed");
      return EBOS_ERR_LAUNCH;
    }
    return EBOS_OK;
  }
  FilterScratch fs = carve(scratch, n, 1, 1);
  const dim3 blk(kFiltBlock), g(stream_grid(n, kFiltBlock));
  mask_to_i32_kernel<<<g, blk, 0, s>>>(mask, n, fs.vals_a);
  scan_exclusive_i32(fs.vals_a, n, n_out, fs.block_sums, s);
  compact_kernel<<<g, blk, 0, s>>>(make_source(src, 1, 1), n, mask, fs.vals_a, events_out, col_out, row_out, t_out, pol_out);
  EBOS_CHECK_LAUNCH("ebos_filter_compact");
  return EBOS_OK;
}

}  // extern "C"
