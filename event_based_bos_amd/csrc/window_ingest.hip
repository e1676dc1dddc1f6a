// window_ingest.hip -- the event side of several solver windows in one launch, straight from the raw sensor columns
// (RawEventStore.load_raw: col int16, row int16, t int32 | int64 ticks, pol uint8).
//
// For every window b = [begin_b, end_b) of the columns (the ranges may overlap or be empty) and the CROP rectangle of the solver:
//   pol  [B, 2, H, W] float64   positive / negative event counts per pixel -- create_image_from_events_numpy(ev, "polarity",
//                               sigma = 0) of the cropped window: raw events lie on integer pixels, their bilinear weights are
//                               exactly (1, 0, 0, 0), so the image is a count and any summation order gives the same bits;
//   mask [B, H, W] uint8        pixels with at least one event (create_eventmask);
//   count, t_min, t_max [B]     the kept events and their first / last time in seconds (ticks / ticks_per_second, float64, as
//                               RawEventStore.load_event converts them): preprocess' period is t_max - t_min.
// "Kept" = inside the CROP rectangle (when there is one) and outside the removal rectangle (when there is one).
//
// Counting is done in integers.  The kept pixels are numbered q = (row - r0) * bw + (col - c0) inside the box = CROP rectangle
// clipped to the sensor; a workgroup owns (window, tile of kTilePixels consecutive q, chunk of kChunk events): it counts the chunk's
// events of its tile in LDS (uint32 per pixel and polarity, ds_add), then adds the non-zero cells to the window's uint32 count
// image with integer atomics -- a stuck pixel's tens of thousands of events meet in LDS, not at one address in memory.  The
// events of a chunk are read once per tile; they are 9 bytes each and stay in L2.  The workgroups of tile 0 also reduce the
// count and the tick range (wave reduction, then one integer atomic per wave).  A second launch turns the counts into pol and
// mask (every pixel of the image is written: nothing to zero first) and the tick range into seconds.
// No floating-point atomic, so two runs give the same bits.
#include "common.h"

namespace ebos {
namespace {

constexpr int kIngestBlock = 512;
constexpr int kTilePixels = 8192;              // x 2 polarities x 4 B = 64 KiB of LDS
constexpr int kChunk = 64 * kIngestBlock;      // events per workgroup and pass
constexpr unsigned long long kCountFloor = 0x8080808080808080ull;   // what hipMemsetAsync(0x80) leaves in the statistics:
constexpr int64_t kTickFloor = (int64_t)kCountFloor;                  // as a tick, a value below any tick or -tick

struct IngestGeom {
  int H, W;
  int has_roi, x0, x1, y0, y1;      // CROP: rows [x0, x1), columns [y0, y1)
  int has_rm, rx0, rx1, ry0, ry1;   // removal rectangle
  int r0, c0, bh, bw;               // the box: CROP clipped to the sensor (the whole sensor without CROP)
};

struct IngestStats {   // per window, in scratch
  unsigned long long count;
  long long max_t, max_neg_t;
  long long pad;
};

__device__ __forceinline__ int64_t load_ticks(const void* t, int t64, int64_t i) {
  return t64 ? static_cast<const int64_t*>(t)[i] : (int64_t) static_cast<const int32_t*>(t)[i];
}

__device__ __forceinline__ void window_range(const int64_t* __restrict__ ranges, int b, int64_t n_total, int64_t& lo, int64_t& hi) {
  lo = ranges[2 * b];
  hi = ranges[2 * b + 1];
  lo = lo < 0 ? 0 : (lo > n_total ? n_total : lo);
  hi = hi < lo ? lo : (hi > n_total ? n_total : hi);
}

__global__ void __launch_bounds__(kIngestBlock)
ingest_count_kernel(const int16_t* __restrict__ col, const int16_t* __restrict__ row, const void* __restrict__ t, int t64,
                    const uint8_t* __restrict__ pol, int64_t n_total, const int64_t* __restrict__ ranges, IngestGeom g,
                    uint32_t* __restrict__ counts, IngestStats* __restrict__ stats) {
  __shared__ uint32_t cell[2 * kTilePixels];
  const int b = blockIdx.z, tile = blockIdx.y;
  int64_t lo, hi;
  window_range(ranges, b, n_total, lo, hi);
  if (lo + (int64_t)blockIdx.x * kChunk >= hi) return;   // (uniform over the workgroup)
  const int box = g.bh * g.bw;
  const int q0 = tile * kTilePixels;
  const bool first_tile = tile == 0;
  for (int k = threadIdx.x; k < 2 * kTilePixels; k += kIngestBlock) cell[k] = 0u;
  __syncthreads();
  unsigned long long kept = 0;
  long long tmax = kTickFloor, tnmax = kTickFloor;
  bool hit = false;
  for (int64_t base = lo + (int64_t)blockIdx.x * kChunk; base < hi; base += (int64_t)gridDim.x * kChunk) {
    const int64_t stop = base + kChunk < hi ? base + kChunk : hi;
    for (int64_t i = base + threadIdx.x; i < stop; i += kIngestBlock) {
      const int r = row[i], c = col[i];
      bool keep = !g.has_roi || (r >= g.x0 && r < g.x1 && c >= g.y0 && c < g.y1);
      if (g.has_rm && r >= g.rx0 && r < g.rx1 && c >= g.ry0 && c < g.ry1) keep = false;
      if (!keep) continue;
      if (first_tile) {
        const long long tk = load_ticks(t, t64, i);
        ++kept;
        tmax = tk > tmax ? tk : tmax;
        tnmax = -tk > tnmax ? -tk : tnmax;
      }
      const int rr = r - g.r0, cc = c - g.c0;
      if (rr < 0 || rr >= g.bh || cc < 0 || cc >= g.bw) continue;   // kept, but not on the sensor: no pixel to count on
      const int q = rr * g.bw + cc - q0;
      if (q < 0 || q >= kTilePixels) continue;
      atomicAdd(&cell[(pol[i] != 0 ? 0 : kTilePixels) + q], 1u);   // channel 0 <- p > 0, as the polarity splat
      hit = true;
    }
  }
  if (first_tile) {       // all lanes take part in the shuffles
    const unsigned long long k = wave_sum(kept);
    const long long a = wave_max(tmax), n = wave_max(tnmax);
    if ((threadIdx.x & (kWave - 1)) == 0 && k != 0ull) {
      atomicAdd(&stats[b].count, k);   // (starts at kCountFloor)
      atomicMax(&stats[b].max_t, a);
      atomicMax(&stats[b].max_neg_t, n);
    }
  }
  if (!__syncthreads_or(hit)) return;   // nothing of this chunk fell into this tile
  uint32_t* dst = counts + (size_t)b * 2 * box;
  const int lim = box - q0 < kTilePixels ? box - q0 : kTilePixels;
  for (int k = threadIdx.x; k < 2 * kTilePixels; k += kIngestBlock) {
    const uint32_t v = cell[k];
    const int ch = k >= kTilePixels, q = k - ch * kTilePixels;
    if (v != 0u && q < lim) atomicAdd(&dst[(size_t)ch * box + q0 + q], v);
  }
}

__global__ void __launch_bounds__(256)
ingest_finish_kernel(const uint32_t* __restrict__ counts, const IngestStats* __restrict__ stats, IngestGeom g, double tps,
                     double* __restrict__ pol_out, uint8_t* __restrict__ mask_out, int64_t* __restrict__ count_out,
                     double* __restrict__ tmin_out, double* __restrict__ tmax_out) {
  const int b = blockIdx.y;
  const int64_t P = (int64_t)g.H * g.W;
  const int box = g.bh * g.bw;
  const uint32_t* src = counts + (size_t)b * 2 * box;
  double* dst = pol_out + (size_t)b * 2 * P;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(p / g.W), c = (int)(p - (int64_t)r * g.W);
    const int rr = r - g.r0, cc = c - g.c0;
    uint32_t pos = 0u, neg = 0u;
    if (rr >= 0 && rr < g.bh && cc >= 0 && cc < g.bw) {
      const int q = rr * g.bw + cc;
      pos = src[q];
      neg = src[box + q];
    }
    dst[p] = (double)pos;
    dst[P + p] = (double)neg;
    mask_out[(size_t)b * P + p] = (pos | neg) != 0u;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const IngestStats s = stats[b];
    const unsigned long long n = s.count - kCountFloor;
    count_out[b] = (int64_t)n;
    tmin_out[b] = n ? (double)(-s.max_neg_t) / tps : 0.0;
    tmax_out[b] = n ? (double)s.max_t / tps : 0.0;
  }
}

bool make_geom(int H, int W, int has_roi, int xmin, int xmax, int ymin, int ymax, int has_rm, int rx0, int rx1, int ry0, int ry1,
               IngestGeom* g) {
  g->H = H;
  g->W = W;
  g->has_roi = has_roi != 0;
  g->x0 = xmin, g->x1 = xmax, g->y0 = ymin, g->y1 = ymax;
  g->has_rm = has_rm != 0;
  g->rx0 = rx0, g->rx1 = rx1, g->ry0 = ry0, g->ry1 = ry1;
  const int r0 = has_roi ? (xmin < 0 ? 0 : xmin) : 0, r1 = has_roi ? (xmax > H ? H : xmax) : H;
  const int c0 = has_roi ? (ymin < 0 ? 0 : ymin) : 0, c1 = has_roi ? (ymax > W ? W : ymax) : W;
  g->r0 = r0;
  g->c0 = c0;
  g->bh = r1 > r0 ? r1 - r0 : 0;
  g->bw = c1 > c0 ? c1 - c0 : 0;
  if (g->bh == 0 || g->bw == 0) g->bh = g->bw = 0;
  return true;
}

inline size_t ingest_align(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace
}  // namespace ebos

extern "C" {

size_t ebos_window_ingest_scratch_bytes(int B, int H, int W, int has_roi, int xmin, int xmax, int ymin, int ymax) {
  using namespace ebos;
  if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31) - 1) return 0;
  IngestGeom g;
  make_geom(H, W, has_roi, xmin, xmax, ymin, ymax, 0, 0, 0, 0, 0, &g);
  return ingest_align((size_t)B * sizeof(IngestStats)) + ingest_align((size_t)B * 2 * g.bh * g.bw * sizeof(uint32_t)) + 256;
}

int ebos_window_ingest_raw_batch(const int16_t* col, const int16_t* row, const void* t, int t_is_64, const uint8_t* pol,
                                 int64_t n_total, double ticks_per_second, const int64_t* ranges, int B, int64_t max_len, int H,
                                 int W, int has_roi, int xmin, int xmax, int ymin, int ymax, int has_remove, int rm_x0, int rm_x1,
                                 int rm_y0, int rm_y1, double* pol_out, uint8_t* mask_out, int64_t* count_out, double* tmin_out,
                                 double* tmax_out, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  const char* who = "ebos_window_ingest_raw_batch";
  EBOS_REQUIRE(B > 0 && B <= 65535, "%s: B = %d outside 1 .. 65535", who, B);
  EBOS_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) - 1, "%s: bad sensor size %d x %d", who, H, W);
  EBOS_REQUIRE(n_total >= 0 && max_len >= 0 && max_len <= n_total, "%s: n_total = %lld, max_len = %lld", who, (long long)n_total,
               (long long)max_len);
  EBOS_REQUIRE((col && row && t && pol) || n_total == 0, "%s: NULL raw column", who);
  EBOS_REQUIRE(ticks_per_second > 0.0, "%s: ticks_per_second must be > 0", who);
  EBOS_REQUIRE(ranges && pol_out && mask_out && count_out && tmin_out && tmax_out && scratch, "%s: NULL buffer", who);
  EBOS_REQUIRE(!has_roi || (xmin <= xmax && ymin <= ymax), "%s: bad CROP rectangle", who);
  const size_t need = ebos_window_ingest_scratch_bytes(B, H, W, has_roi, xmin, xmax, ymin, ymax);
  if (scratch_bytes < need) {
    set_error("%s: scratch too small (%zu < %zu)", who, scratch_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  IngestGeom g;
  make_geom(H, W, has_roi, xmin, xmax, ymin, ymax, has_remove, rm_x0, rm_x1, rm_y0, rm_y1, &g);
  const int box = g.bh * g.bw;
  EBOS_REQUIRE((box + kTilePixels - 1) / kTilePixels <= 65535, "%s: the CROP rectangle holds too many pixels (%d)", who, box);
  hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(scratch);
  IngestStats* stats = reinterpret_cast<IngestStats*>(base);
  const size_t stats_bytes = ingest_align((size_t)B * sizeof(IngestStats));
  uint32_t* counts = reinterpret_cast<uint32_t*>(base + stats_bytes);
  const size_t count_bytes = (size_t)B * 2 * box * sizeof(uint32_t);
  // every byte 0x80: the tick maxima start below any tick, the event count at kCountFloor
  bool ok = hipMemsetAsync(stats, 0x80, (size_t)B * sizeof(IngestStats), s) == hipSuccess;
  if (count_bytes) ok = ok && hipMemsetAsync(counts, 0, count_bytes, s) == hipSuccess;
  if (!ok) {
    set_error("%s: hipMemsetAsync failed", who);
    return EBOS_ERR_LAUNCH;
  }
  if (max_len > 0 && n_total > 0) {
    const int tiles = box > 0 ? (box + kTilePixels - 1) / kTilePixels : 1;
    int64_t chunks = (max_len + kChunk - 1) / kChunk;
    if (chunks > 4096) chunks = 4096;   // (longer windows: the chunk loop strides over the grid)
    ingest_count_kernel<<<dim3((unsigned)chunks, (unsigned)tiles, (unsigned)B), dim3(kIngestBlock), 0, s>>>(
        col, row, t, t_is_64 != 0, pol, n_total, ranges, g, counts, stats);
  }
  const int fx = stream_grid((int64_t)H * W, 256, 1024);
  ingest_finish_kernel<<<dim3(fx, B), dim3(256), 0, s>>>(counts, stats, g, ticks_per_second, pol_out, mask_out, count_out,
                                                        tmin_out, tmax_out);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

}  // extern "C"
