// splat_ordered.hip -- the ordered route of the event -> image vote for gfx950: a sorted index of the events by destination cell,
// then one owner per pixel that sums its addends in a fixed order with a plain store.  No atomics on the image, no float atomics
// anywhere: the image is a pure function of the input, bit for bit, call after call, alone or inside a batch.  The atomic route
// (splat_kernels.hip) stays the default; both compute every tap from the same footprint<T>() of common.h.
//
// THE INDEX (ebos_splat_index_build_*).  events [b, n, 4]; event i = row * n + e (32 bit).  Its top-left tap (R, C) = footprint<T>() lies
// in the extended grid R in [-1, h - 1], C in [-1, w - 1] (h, w: the padded image) or the event is dropped: none of its four taps is
// inside, or its coordinates are not finite.  key = ((row * planes + plane) * (h + 1) + R + 1) * (w + 1) + C + 1, planes = 2 and
// plane = (p > 0 ? 0 : 1) for EBOS_SPLAT_POLARITY, else planes = 1.  keys = b * planes * (h + 1) * (w + 1); a dropped event takes the
// key `keys`.  A stable least-significant-digit radix sort (8-bit digits, as many passes as `keys` has bytes) orders the event indices by
// key: per pass a digit histogram per tile of 4096 events, an exclusive scan of the digit-major table, and a scatter whose rank inside
// the tile is the event's position among the tile's events of the same digit (wave ballots, waves in turn).  Nothing depends on the
// order in which anything arrives.  offsets[k] = the first sorted position whose key is >= k (a binary search per key), k = 0 .. keys.
// Within a key the indices ascend; the dropped events stand behind offsets[keys].
//
// THE SUMMATION ORDER (ebos_splat_ordered_*).  One lane owns pixel (row, plane, r, c).  Its addend list is, in this order, the events
// of the cells (r - 1, c - 1), (r - 1, c), (r, c - 1), (r, c), each cell in ascending event index.  The addend of an event of these
// cells is its tap on (r, c), formed as splat_kernel forms it in element type T, every product rounded on its own (-ffp-contract=off):
//     fr * fc * wv,   fr * (1 - fc) * wv,   (1 - fr) * fc * wv,   (1 - fr) * (1 - fc) * wv     (each (x * y) * wv)
// for the four cells, wv = weight[i] or the scalar weight; EBOS_SPLAT_COUNT adds 1 instead.
//   * a list of at most kSplatLongList addends:  s = +0;  s = s + addend, in list order.
//   * a longer list is summed by the pixel's whole wave: lane l forms  p_l = +0;  p_l = p_l + addend[j]  for j = l, l + 64, l + 128, ...
//     ascending; then for off = 32, 16, 8, 4, 2, 1:  p_l = p_l + p_(l + off)  for l < off;  s = p_0.
// The pixel is stored once, with a plain store; a pixel without addends is +0.  The caller does not zero the image.
#include "common.h"

namespace ebos {
namespace {

constexpr int kSplatLongList = 256;  // addend lists longer than this are summed by a whole wave
constexpr int kSortBlock = 256;
constexpr int kSortItems = 16;
constexpr int kSortTile = kSortBlock * kSortItems;  // events per workgroup of a radix pass
constexpr int kDigits = 256;
static_assert(kDigits == kSortBlock, "one thread per digit in the radix kernels");

template <typename T>
struct Ev4;
template <>
struct Ev4<float> {
  using type = float4;
};
template <>
struct Ev4<double> {
  using type = double4;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// sections of the index workspace, 256-byte aligned, in this order (include/ebos_hip.h states the first two)
struct IndexLayout {
  int64_t keys, total;  // number of keys, b * n
  int passes, tiles;
  size_t offsets, idx, keys_a, keys_b, vals_y, table, sums, bytes;
};

inline bool index_layout(int64_t b, int64_t n, int h, int w, int mode, IndexLayout* L) {
  if (b < 1 || b > 65535 || n < 0 || h <= 0 || w <= 0) return false;
  if (mode != EBOS_SPLAT_BILINEAR && mode != EBOS_SPLAT_COUNT && mode != EBOS_SPLAT_POLARITY) return false;
  const int64_t lim = (int64_t)1 << 31;
  if (n >= lim || b * n >= lim) return false;
  const int64_t planes = mode == EBOS_SPLAT_POLARITY ? 2 : 1;
  const int64_t cells = ((int64_t)h + 1) * ((int64_t)w + 1);  // < 2^62
  if (cells >= lim || b * planes * cells >= lim) return false;
  L->keys = b * planes * cells;
  L->total = b * n;
  L->passes = 0;
  for (int64_t k = L->keys; k > 0; k >>= 8) ++L->passes;  // the dropped events' key `keys` is sorted too
  L->tiles = (int)((L->total + kSortTile - 1) / kSortTile);
  const size_t ev = align256((size_t)L->total * 4);
  const size_t table = (size_t)L->tiles * kDigits;
  size_t at = 0;
  L->offsets = at, at += align256((size_t)(L->keys + 1) * 4);
  L->idx = at, at += ev;
  L->keys_a = at, at += ev;
  L->keys_b = at, at += ev;
  L->vals_y = at, at += ev;
  L->table = at, at += align256(table * 4);
  L->sums = at, at += align256(((size_t)scan_blocks((int64_t)table) + 1) * 4);  // + the scan's grand total
  L->bytes = at;
  return true;
}

// ---- index build ---------------------------------------------------------------------------------------------------------------
template <typename T, bool POLARITY>
__global__ void __launch_bounds__(256)
splat_keys_kernel(const T* __restrict__ events, T eps, int64_t total, int64_t n, int h, int w, int pad_h, int pad_w, uint32_t n_keys,
                  uint32_t* __restrict__ keys) {
  const auto* ev = reinterpret_cast<const typename Ev4<T>::type*>(events);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const auto e = ev[i];
    const Footprint<T> f = footprint<T>(e.x, e.y, eps, pad_h, pad_w);
    const bool keep = f.finite && f.R >= -1 && f.R <= h - 1 && f.C >= -1 && f.C <= w - 1;
    uint32_t img = (uint32_t)(i / n);
    if (POLARITY) img = img * 2u + ((e.w > T(0)) ? 0u : 1u);
    keys[i] = keep ? (img * (uint32_t)(h + 1) + (uint32_t)(f.R + 1)) * (uint32_t)(w + 1) + (uint32_t)(f.C + 1) : n_keys;
  }
}

// digit histogram of one tile -> table[digit * tiles + tile] (integer counts: the same whatever the order of the adds)
__global__ void __launch_bounds__(kSortBlock)
radix_hist_kernel(const uint32_t* __restrict__ keys, int64_t total, int shift, int tiles, int32_t* __restrict__ table) {
  __shared__ int32_t hist[kDigits];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tile0 = (int64_t)blockIdx.x * kSortTile;
  for (int k = 0; k < kSortItems; ++k) {
    const int64_t j = tile0 + k * kSortBlock + threadIdx.x;
    if (j < total) atomicAdd(&hist[(keys[j] >> shift) & (kDigits - 1)], 1);
  }
  __syncthreads();
  table[(int64_t)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

// stable scatter of one tile: position = scanned table entry of (digit, tile) + the number of earlier events of the tile with the
// same digit.  "Earlier" is the position j in the tile: rounds of 256 in turn, inside a round the four waves in turn, inside a wave
// the lanes below (a ballot per digit bit).  vals_in == NULL: the value of position j is j (the first pass).
__global__ void __launch_bounds__(kSortBlock)
radix_scatter_kernel(const uint32_t* __restrict__ keys_in, const int32_t* __restrict__ vals_in, int64_t total, int shift, int tiles,
                     const int32_t* __restrict__ table, uint32_t* __restrict__ keys_out, int32_t* __restrict__ vals_out) {
  __shared__ int32_t next[kDigits];  // where the tile's next event of a digit goes
  next[threadIdx.x] = table[(int64_t)threadIdx.x * tiles + blockIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t tile0 = (int64_t)blockIdx.x * kSortTile;
  for (int k = 0; k < kSortItems; ++k) {
    const int64_t j = tile0 + k * kSortBlock + threadIdx.x;
    const bool valid = j < total;
    const uint32_t key = valid ? keys_in[j] : 0u;
    const int32_t val = valid ? (vals_in ? vals_in[j] : (int32_t)j) : 0;
    const int d = (int)((key >> shift) & (kDigits - 1));
    unsigned long long same = __ballot(valid);  // the valid lanes of this wave with this lane's digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool set = (d >> bit) & 1;
      const unsigned long long m = __ballot(valid && set);
      same &= set ? m : ~m;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull));
    const int leader = valid ? __ffsll((long long)same) - 1 : lane;
    int32_t pos = 0;
    for (int wv = 0; wv < kSortBlock / kWave; ++wv) {
      if (wave == wv) {  // wave-uniform
        int32_t first = 0;
        if (valid && lane == leader) {  // one lane per digit of the wave
          first = next[d];
          next[d] = first + __popcll(same);
        }
        pos = __shfl(first, leader, kWave) + rank;
      }
      __syncthreads();
    }
    if (valid) {
      keys_out[pos] = key;
      vals_out[pos] = val;
    }
  }
}

// offsets[k] = first position of the sorted keys that is >= k, k = 0 .. n_keys
__global__ void __launch_bounds__(256)
splat_offsets_kernel(const uint32_t* __restrict__ sorted, int64_t total, int64_t n_keys, int32_t* __restrict__ offsets) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k <= n_keys; k += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = total;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sorted[mid] < (uint32_t)k) lo = mid + 1; else hi = mid;
    }
    offsets[k] = (int32_t)lo;
  }
}

template <typename T>
int index_build_impl(const T* events, int mode, double eps, int64_t b, int64_t n, int h, int w, int pad_h, int pad_w, void* index,
                     size_t index_bytes, ebos_stream_t stream) {
  IndexLayout L;
  EBOS_REQUIRE(b >= 1 && b <= 65535 && n >= 0 && h > 0 && w > 0 && pad_h >= 0 && pad_w >= 0,
               "ebos_splat_index_build: bad sizes b=%lld n=%lld h=%d w=%d", (long long)b, (long long)n, h, w);
  EBOS_REQUIRE(index_layout(b, n, h, w, mode, &L),
               "ebos_splat_index_build: mode %d unknown, or b*n or b*planes*(h+1)*(w+1) reaches 2^31 (b=%lld n=%lld h=%d w=%d)", mode,
               (long long)b, (long long)n, h, w);
  EBOS_REQUIRE(index != nullptr && index_bytes >= L.bytes, "ebos_splat_index_build: index workspace too small (%zu < %zu)",
               index ? index_bytes : (size_t)0, L.bytes);
  EBOS_REQUIRE(events != nullptr || n == 0, "ebos_splat_index_build: events is NULL");
  hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(index);
  int32_t* offsets = reinterpret_cast<int32_t*>(base + L.offsets);
  if (L.total == 0) {
    if (hipMemsetAsync(offsets, 0, (size_t)(L.keys + 1) * 4, s) != hipSuccess) {
      set_error("ebos_splat_index_build: hipMemsetAsync failed");
      return EBOS_ERR_LAUNCH;
    }
    return EBOS_OK;
  }
  uint32_t* kbuf[2] = {reinterpret_cast<uint32_t*>(base + L.keys_a), reinterpret_cast<uint32_t*>(base + L.keys_b)};
  int32_t* idx = reinterpret_cast<int32_t*>(base + L.idx);
  int32_t* vals_y = reinterpret_cast<int32_t*>(base + L.vals_y);
  int32_t* table = reinterpret_cast<int32_t*>(base + L.table);
  int32_t* sums = reinterpret_cast<int32_t*>(base + L.sums);
  const int64_t table_n = (int64_t)L.tiles * kDigits;
  const T e = static_cast<T>(eps);
  if (mode == EBOS_SPLAT_POLARITY)
    splat_keys_kernel<T, true><<<stream_grid(L.total, 256), 256, 0, s>>>(events, e, L.total, n, h, w, pad_h, pad_w, (uint32_t)L.keys,
                                                                         kbuf[0]);
  else
    splat_keys_kernel<T, false><<<stream_grid(L.total, 256), 256, 0, s>>>(events, e, L.total, n, h, w, pad_h, pad_w, (uint32_t)L.keys,
                                                                          kbuf[0]);
  for (int p = 0; p < L.passes; ++p) {
    // the values alternate between the index proper and vals_y so that the last pass writes the index
    int32_t* out = ((L.passes - 1 - p) & 1) ? vals_y : idx;
    const int32_t* in = p == 0 ? nullptr : (out == idx ? vals_y : idx);
    radix_hist_kernel<<<L.tiles, kSortBlock, 0, s>>>(kbuf[p & 1], L.total, 8 * p, L.tiles, table);
    scan_exclusive_i32(table, table_n, sums + scan_blocks(table_n), sums, s);
    radix_scatter_kernel<<<L.tiles, kSortBlock, 0, s>>>(kbuf[p & 1], in, L.total, 8 * p, L.tiles, table, kbuf[(p + 1) & 1], out);
  }
  splat_offsets_kernel<<<stream_grid(L.keys + 1, 256), 256, 0, s>>>(kbuf[L.passes & 1], L.total, L.keys, offsets);
  EBOS_CHECK_LAUNCH("ebos_splat_index_build");
  return EBOS_OK;
}

// ---- owner gather --------------------------------------------------------------------------------------------------------------
// the tap of event i on the pixel that lies (1 - q / 2) rows and (1 - q % 2) columns from the event's top-left tap:
// q = 0: cell (r - 1, c - 1), 1: (r - 1, c), 2: (r, c - 1), 3: (r, c)
template <typename T, int MODE>
__device__ __forceinline__ T splat_addend(const typename Ev4<T>::type* __restrict__ ev, const T* __restrict__ wt, T weight_scalar, T eps,
                                          int pad_h, int pad_w, int32_t i, int q) {
  if (MODE == EBOS_SPLAT_COUNT) return T(1);
  const auto e = ev[i];
  const Footprint<T> f = footprint<T>(e.x, e.y, eps, pad_h, pad_w);
  const T wv = wt ? wt[i] : weight_scalar;
  const T a = T(1) - f.fr, b = T(1) - f.fc;
  const T x = (q & 2) ? a : f.fr, y = (q & 1) ? b : f.fc;
  return x * y * wv;
}

template <typename T, int MODE>
__global__ void __launch_bounds__(256)
splat_ordered_kernel(const T* __restrict__ events, const T* __restrict__ weight, T weight_scalar, T eps, int64_t pixels, int h, int w,
                     int pad_h, int pad_w, const int32_t* __restrict__ offsets, const int32_t* __restrict__ idx, T* __restrict__ image) {
  const auto* ev = reinterpret_cast<const typename Ev4<T>::type*>(events);
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t hw = (int64_t)h * w, cells = (int64_t)(h + 1) * (w + 1);
  const int64_t pix = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool valid = pix < pixels;
  // the cells (r - 1, c - 1), (r - 1, c) are the keys k0, k0 + 1 and (r, c - 1), (r, c) the keys k0 + w + 1, k0 + w + 2
  int32_t s0 = 0, s1 = 0, s2 = 0, t0 = 0, t1 = 0, t2 = 0;  // runs [s0, s1) [s1, s2) [t0, t1) [t1, t2) of idx
  if (valid) {
    const int64_t img = pix / hw, rem = pix - img * hw;
    const int r = (int)(rem / w), c = (int)(rem - (int64_t)r * w);
    const int64_t k0 = img * cells + (int64_t)r * (w + 1) + c;
    s0 = offsets[k0], s1 = offsets[k0 + 1], s2 = offsets[k0 + 2];
    t0 = offsets[k0 + w + 1], t1 = offsets[k0 + w + 2], t2 = offsets[k0 + w + 3];
  }
  const int len = (s2 - s0) + (t2 - t0);
  const bool is_long = len > kSplatLongList;
  T sum = T(0);
  if (valid && !is_long) {
    for (int32_t j = s0; j < s1; ++j) sum = sum + splat_addend<T, MODE>(ev, weight, weight_scalar, eps, pad_h, pad_w, idx[j], 0);
    for (int32_t j = s1; j < s2; ++j) sum = sum + splat_addend<T, MODE>(ev, weight, weight_scalar, eps, pad_h, pad_w, idx[j], 1);
    for (int32_t j = t0; j < t1; ++j) sum = sum + splat_addend<T, MODE>(ev, weight, weight_scalar, eps, pad_h, pad_w, idx[j], 2);
    for (int32_t j = t1; j < t2; ++j) sum = sum + splat_addend<T, MODE>(ev, weight, weight_scalar, eps, pad_h, pad_w, idx[j], 3);
  }
  // long lists, one after the other, by the whole wave (every lane of the wave is here: no lane has left the kernel)
  unsigned long long todo = __ballot(valid && is_long);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int32_t a0 = __shfl(s0, src, kWave), a1 = __shfl(s1, src, kWave), a2 = __shfl(s2, src, kWave);
    const int32_t b0 = __shfl(t0, src, kWave), b1 = __shfl(t1, src, kWave), b2 = __shfl(t2, src, kWave);
    const int32_t first = a2 - a0, n_list = first + (b2 - b0);
    T part = T(0);
    for (int32_t j = lane; j < n_list; j += kWave) {
      const int32_t at = j < first ? a0 + j : b0 + (j - first);  // position in idx
      const int q = j < first ? (at < a1 ? 0 : 1) : (at < b1 ? 2 : 3);
      part = part + splat_addend<T, MODE>(ev, weight, weight_scalar, eps, pad_h, pad_w, idx[at], q);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const T other = __shfl_down(part, off, kWave);
      if (lane < off) part = part + other;
    }
    const T total = __shfl(part, 0, kWave);
    if (lane == src) sum = total;
  }
  if (valid) image[pix] = sum;
}

template <typename T>
int splat_ordered_impl(const T* events, const T* weight, double weight_scalar, int mode, double eps, int64_t b, int64_t n, int h, int w,
                       int pad_h, int pad_w, const void* index, size_t index_bytes, T* image, ebos_stream_t stream) {
  IndexLayout L;
  EBOS_REQUIRE(b >= 1 && b <= 65535 && n >= 0 && h > 0 && w > 0 && pad_h >= 0 && pad_w >= 0,
               "ebos_splat_ordered: bad sizes b=%lld n=%lld h=%d w=%d", (long long)b, (long long)n, h, w);
  EBOS_REQUIRE(index_layout(b, n, h, w, mode, &L),
               "ebos_splat_ordered: mode %d unknown, or b*n or b*planes*(h+1)*(w+1) reaches 2^31 (b=%lld n=%lld h=%d w=%d)", mode,
               (long long)b, (long long)n, h, w);
  EBOS_REQUIRE(index != nullptr && index_bytes >= L.bytes, "ebos_splat_ordered: index workspace too small (%zu < %zu)",
               index ? index_bytes : (size_t)0, L.bytes);
  EBOS_REQUIRE(image != nullptr, "ebos_splat_ordered: image is NULL");
  EBOS_REQUIRE(events != nullptr || n == 0, "ebos_splat_ordered: events is NULL");
  const char* base = static_cast<const char*>(index);
  const int32_t* offsets = reinterpret_cast<const int32_t*>(base + L.offsets);
  const int32_t* idx = reinterpret_cast<const int32_t*>(base + L.idx);
  const int64_t pixels = b * (mode == EBOS_SPLAT_POLARITY ? 2 : 1) * (int64_t)h * w;  // < keys < 2^31
  const unsigned grid = (unsigned)((pixels + 255) / 256);
  hipStream_t s = as_stream(stream);
  const T ws = static_cast<T>(weight_scalar), e = static_cast<T>(eps);
  switch (mode) {
    case EBOS_SPLAT_BILINEAR:
      splat_ordered_kernel<T, EBOS_SPLAT_BILINEAR><<<grid, 256, 0, s>>>(events, weight, ws, e, pixels, h, w, pad_h, pad_w, offsets, idx,
                                                                        image);
      break;
    case EBOS_SPLAT_COUNT:
      splat_ordered_kernel<T, EBOS_SPLAT_COUNT><<<grid, 256, 0, s>>>(events, weight, ws, e, pixels, h, w, pad_h, pad_w, offsets, idx,
                                                                     image);
      break;
    default:
      splat_ordered_kernel<T, EBOS_SPLAT_POLARITY><<<grid, 256, 0, s>>>(events, weight, ws, e, pixels, h, w, pad_h, pad_w, offsets, idx,
                                                                        image);
      break;
  }
  EBOS_CHECK_LAUNCH("ebos_splat_ordered");
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {
size_t ebos_splat_index_bytes(int64_t b, int64_t n, int h, int w, int mode) {
  ebos::IndexLayout L;
  return ebos::index_layout(b, n, h, w, mode, &L) ? L.bytes : 0;
}
int ebos_splat_index_build_f32(const float* events, int mode, double eps, int64_t b, int64_t n, int h, int w, int pad_h, int pad_w,
                               void* index, size_t index_bytes, ebos_stream_t stream) {
  return ebos::index_build_impl<float>(events, mode, eps, b, n, h, w, pad_h, pad_w, index, index_bytes, stream);
}
int ebos_splat_index_build_f64(const double* events, int mode, double eps, int64_t b, int64_t n, int h, int w, int pad_h, int pad_w,
                               void* index, size_t index_bytes, ebos_stream_t stream) {
  return ebos::index_build_impl<double>(events, mode, eps, b, n, h, w, pad_h, pad_w, index, index_bytes, stream);
}
int ebos_splat_ordered_f32(const float* events, const float* weight, double weight_scalar, int mode, double eps, int64_t b, int64_t n,
                           int h, int w, int pad_h, int pad_w, const void* index, size_t index_bytes, float* image,
                           ebos_stream_t stream) {
  return ebos::splat_ordered_impl<float>(events, weight, weight_scalar, mode, eps, b, n, h, w, pad_h, pad_w, index, index_bytes, image,
                                         stream);
}
int ebos_splat_ordered_f64(const double* events, const double* weight, double weight_scalar, int mode, double eps, int64_t b, int64_t n,
                           int h, int w, int pad_h, int pad_w, const void* index, size_t index_bytes, double* image,
                           ebos_stream_t stream) {
  return ebos::splat_ordered_impl<double>(events, weight, weight_scalar, mode, eps, b, n, h, w, pad_h, pad_w, index, index_bytes, image,
                                          stream);
}
}  // extern "C"
