// evt3.hip -- Prophesee EVT 3.0 word streams (the .raw recordings of the reference, src/data_loader/ccs.py:171) decoded on the
// device.  The format and the entry points: include/ebos_hip.h; the state algebra: evt3_core.h.
//
// EVT3 is stateful -- time high, time low, row, vector base and polarity are set by separate 16-bit words, and one vector word fires
// up to twelve events -- but what a stretch of words does to that state is a small record that composes (evt3::Xf), so the decode is
// a scan in three passes over chunks of kChunk words, one 256-thread workgroup per chunk, eight consecutive words per thread:
//   1. summary  every thread folds its words into an Xf, the workgroup combines them in order: one Xf per chunk;
//   2. scan     ONE workgroup combines the chunks' records in order from the carried-in state and leaves, per chunk, the incoming
//               state and the exclusive event and trigger offsets (64-bit: a slab can yield 12 events per word), plus the slab's
//               totals and the carry-out;
//   3. emit     every thread folds its words again, an exclusive scan over the workgroup gives it its own incoming state and
//               offsets, and it decodes its eight words from there; the chunk's events are staged in LDS and stored to their final
//               places by the whole workgroup, consecutive lanes on consecutive elements.
// Integer arithmetic only, no atomics: stream order, the same bytes every run.  Every store is guarded by the caller's capacity.
#include "common.h"
#include "evt3_core.h"

namespace ebos {
namespace {

using evt3::Xf;

constexpr int kBlock = 256;
// words per thread, a multiple of 8 (whole 16-byte loads).  16 halves the summary and the scan pass (0.12 + 0.23 against 0.22 + 0.45 ms
// on 64 M words) and doubles the emit pass (1.58 against 0.86 ms: 204 registers a thread)
constexpr int kPerThread = 8;
static_assert(kPerThread % 8 == 0, "whole 16-byte loads");
constexpr int kChunk = kBlock * kPerThread;
constexpr int kWaves = kBlock / kWave;
constexpr int kScanBlock = 1024;  // the one workgroup of the scan pass
constexpr int kStage = 4096;      // events the emit pass stages in LDS at a time (13 B each)
constexpr int64_t kMaxWords = (int64_t)1 << 30;

struct ChunkIn {
  ebos_evt3_state s;  // the state before the chunk's first word
  long long ev, tr;   // events / triggers of the slab before the chunk
};
static_assert(sizeof(Xf) % 8 == 0 && sizeof(ChunkIn) % 8 == 0, "scratch arrays of 8-byte aligned records");

// an Xf through a lane exchange, field by field (f: a value of lane -> the value of another lane)
template <typename F>
__device__ __forceinline__ evt3::Part exchange(const evt3::Part& p, F f) {
  evt3::Part r;
  r.ev = f(p.ev);
  r.tr = f(p.tr);
  r.tl = f(p.tl);
  r.y = f(p.y);
  r.base = f(p.base);
  r.bx = f(p.bx);
  r.pol = f(p.pol);
  r.reserved = 0;
  return r;
}
template <typename F>
__device__ __forceinline__ Xf exchange(const Xf& x, F f) {
  Xf r;
  r.a = exchange(x.a, f);
  r.has_th = f(x.has_th);
  r.first_th = f(x.first_th);
  r.last_th = f(x.last_th);
  r.wraps = f(x.wraps);
  r.b = exchange(x.b, f);
  return r;
}
__device__ __forceinline__ Xf shfl_up_xf(const Xf& x, int off) {
  return exchange(x, [off](auto v) { return __shfl_up(v, off, kWave); });
}
__device__ __forceinline__ Xf shfl_xf(const Xf& x, int lane) {
  return exchange(x, [lane](auto v) { return __shfl(v, lane, kWave); });
}

// inclusive scan of one Xf per lane over the wave, in lane order
__device__ __forceinline__ Xf wave_scan_inclusive(const Xf& mine) {
  const int lane = threadIdx.x & (kWave - 1);
  Xf inc = mine;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const Xf o = shfl_up_xf(inc, off);
    if (lane >= off) inc = evt3::then(o, inc);
  }
  return inc;
}

// Exclusive scan of one Xf per thread over a workgroup of kWaves waves, in thread order; `total` = all of them.  waves: kWaves
// records of LDS.
template <int kWaves>
__device__ __forceinline__ Xf block_scan_exclusive(const Xf& mine, Xf* waves, Xf& total) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const Xf inc = wave_scan_inclusive(mine);
  if (lane == kWave - 1) waves[wid] = inc;
  __syncthreads();
  Xf exc = shfl_up_xf(inc, 1);
  if (lane == 0) exc = evt3::identity();
  Xf pre = evt3::identity();
  total = evt3::identity();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const Xf t = waves[w];
    if (w < wid) pre = evt3::then(pre, t);
    total = evt3::then(total, t);
  }
  __syncthreads();
  return evt3::then(pre, exc);
}

// the thread's words: word k of thread t of chunk c is words[c * kChunk + t * kPerThread + k]; past the slab's end: 0xF000 (ignored)
__device__ __forceinline__ void load_words(const uint16_t* __restrict__ words, int64_t n_words, int aligned16, unsigned (&w)[kPerThread]) {
  const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kPerThread;
  if (aligned16 && base + kPerThread <= n_words) {
#pragma unroll
    for (int v = 0; v < kPerThread / 8; ++v) {
      const uint4 q = *reinterpret_cast<const uint4*>(words + base + 8 * v);  // (base is a multiple of 8 words = 16 B)
      const unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[8 * v + 2 * k] = d[k] & 0xFFFFu;
        w[8 * v + 2 * k + 1] = d[k] >> 16;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) w[k] = base + k < n_words ? (unsigned)words[base + k] : 0xF000u;
  }
}

__device__ __forceinline__ Xf fold_words(const unsigned (&w)[kPerThread]) {
  Xf x;
  evt3::Part cur;
  evt3::fold_start(x, cur);
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) evt3::fold_word(x, cur, w[k]);
  evt3::fold_finish(x, cur);
  return x;
}

__global__ __launch_bounds__(kBlock) void evt3_summary_kernel(const uint16_t* __restrict__ words, int64_t n_words, int aligned16,
                                                              Xf* __restrict__ sums) {
  __shared__ Xf waves[kWaves];
  unsigned w[kPerThread];
  load_words(words, n_words, aligned16, w);
  Xf total;
  block_scan_exclusive<kWaves>(fold_words(w), waves, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup.  A wave owns a contiguous run of tiles of 64 chunks and walks it twice with one chunk per lane (consecutive lanes
// read and write consecutive records): first for the run's total, then, with the totals of the waves before it, for every chunk's
// incoming state and offsets.
__global__ __launch_bounds__(kScanBlock) void evt3_scan_kernel(const Xf* __restrict__ sums, int64_t n_chunks, const ebos_evt3_state* carry_in,
                                                               ebos_evt3_state* carry_out, int64_t* totals, ChunkIn* __restrict__ cin) {
  constexpr int kScanWaves = kScanBlock / kWave;
  __shared__ Xf waves[kScanWaves];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  ebos_evt3_state s = ebos_evt3_state{0, 0, 0, 0, 0, 0, 0};
  if (carry_in) s = *carry_in;
  const int64_t tiles = (n_chunks + kWave - 1) / kWave, per = (tiles + kScanWaves - 1) / kScanWaves;
  const int64_t first = (int64_t)wid * per;
  const int64_t lo = first < tiles ? first : tiles, hi = lo + per < tiles ? lo + per : tiles;
  Xf run = evt3::identity();
  for (int64_t tile = lo; tile < hi; ++tile) {
    const int64_t c = tile * kWave + lane;
    const Xf inc = wave_scan_inclusive(c < n_chunks ? sums[c] : evt3::identity());
    run = evt3::then(run, shfl_xf(inc, kWave - 1));
  }
  if (lane == 0) waves[wid] = run;
  __syncthreads();  // (every thread has read *carry_in before one writes *carry_out)
  Xf pre = evt3::identity();
  for (int w = 0; w < wid; ++w) pre = evt3::then(pre, waves[w]);
  long long ev = 0, tr = 0;
  evt3::apply(s, pre, ev, tr);
  for (int64_t tile = lo; tile < hi; ++tile) {
    const int64_t c = tile * kWave + lane;
    const Xf inc = wave_scan_inclusive(c < n_chunks ? sums[c] : evt3::identity());
    Xf exc = shfl_up_xf(inc, 1);
    if (lane == 0) exc = evt3::identity();
    ChunkIn in;
    in.s = s;
    in.ev = ev;
    in.tr = tr;
    evt3::apply(in.s, exc, in.ev, in.tr);
    if (c < n_chunks) cin[c] = in;
    evt3::apply(s, shfl_xf(inc, kWave - 1), ev, tr);
  }
  if (threadIdx.x == kScanBlock - 1) {  // (the last wave's tiles are the slab's last ones, or none: s, ev, tr are the slab's)
    *carry_out = s;
    totals[0] = ev;
    totals[1] = tr;
  }
}

// The emit pass's sink.  A thread's events are consecutive in the output but few, so stores straight from the threads would touch
// a cache line per lane: the chunk's events go through LDS instead, kStage at a time (event number `lo` of the chunk onwards), and
// the workgroup copies a full stage out with consecutive lanes on consecutive elements.  Triggers are rare and stored directly, in
// the first stage's walk only.
struct Stage {
  int16_t x[kStage];
  int16_t y[kStage];
  int64_t t[kStage];
  uint8_t p[kStage];
};
struct Sink {
  Stage* stage;
  int64_t* trig_t;
  uint8_t* trig_value;
  uint8_t* trig_id;
  int ev;  // the event's number inside the chunk
  int lo;  // first event number of the stage being filled
  long long tr, tr_cap;
  bool store_triggers;
  __device__ __forceinline__ void event(int ex, int ey, long long et, int ep) {
    const unsigned slot = (unsigned)(ev - lo);  // (below lo: wraps to a large value)
    if (slot < (unsigned)kStage) {
      stage->x[slot] = (int16_t)ex;
      stage->y[slot] = (int16_t)ey;
      stage->t[slot] = et;
      stage->p[slot] = (uint8_t)ep;
    }
    ++ev;
  }
  __device__ __forceinline__ void trigger(long long et, int value, int id) {
    if (store_triggers && tr < tr_cap) {
      trig_t[tr] = et;
      trig_value[tr] = (uint8_t)value;
      trig_id[tr] = (uint8_t)id;
    }
    ++tr;
  }
};

__global__ __launch_bounds__(kBlock) void evt3_emit_kernel(const uint16_t* __restrict__ words, int64_t n_words, int aligned16,
                                                           const ChunkIn* __restrict__ cin, long long ev_cap, long long tr_cap,
                                                           int16_t* __restrict__ x, int16_t* __restrict__ y, int64_t* __restrict__ t,
                                                           uint8_t* __restrict__ p, int64_t* __restrict__ trig_t,
                                                           uint8_t* __restrict__ trig_value, uint8_t* __restrict__ trig_id) {
  __shared__ Xf waves[kWaves];
  __shared__ Stage stage;
  unsigned w[kPerThread];
  load_words(words, n_words, aligned16, w);
  Xf total;
  const Xf pre = block_scan_exclusive<kWaves>(fold_words(w), waves, total);
  const ChunkIn in = cin[blockIdx.x];
  // the chunk's own event count (the same in every thread), and this thread's state and offsets before its first word
  ebos_evt3_state after = in.s;
  long long chunk_ev = 0, chunk_tr = 0;
  evt3::apply(after, total, chunk_ev, chunk_tr);
  ebos_evt3_state mine = in.s;
  long long my_ev = 0, my_tr = in.tr;
  evt3::apply(mine, pre, my_ev, my_tr);
  const int n_ev = (int)chunk_ev;  // (at most 12 kChunk)
  for (int lo = 0; lo == 0 || lo < n_ev; lo += kStage) {
    ebos_evt3_state s = mine;
    Sink out{&stage, trig_t, trig_value, trig_id, (int)my_ev, lo, my_tr, tr_cap, lo == 0};
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) evt3::step(s, w[k], out);
    __syncthreads();
    const int count = n_ev - lo < kStage ? n_ev - lo : kStage;
    for (int i = threadIdx.x; i < count; i += kBlock) {
      const long long g = in.ev + lo + i;
      if (g < ev_cap) {
        x[g] = stage.x[i];
        y[g] = stage.y[i];
        t[g] = stage.t[i];
        p[g] = stage.p[i];
      }
    }
    __syncthreads();
  }
}

inline int64_t chunks_of(int64_t n_words) { return (n_words + kChunk - 1) / kChunk; }
inline size_t scratch_need(int64_t n_words) {
  const int64_t c = chunks_of(n_words) > 0 ? chunks_of(n_words) : 1;
  return (size_t)c * (sizeof(Xf) + sizeof(ChunkIn));
}

}  // namespace
}  // namespace ebos

using namespace ebos;

extern "C" int ebos_evt3_chunk_words(void) { return kChunk; }

extern "C" size_t ebos_evt3_scratch_bytes(int64_t n_words) {
  if (n_words < 0 || n_words > kMaxWords) return 0;
  return scratch_need(n_words);
}

extern "C" int ebos_evt3_scan(const uint16_t* words, int64_t n_words, const ebos_evt3_state* carry_in, ebos_evt3_state* carry_out,
                              int64_t* totals, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(n_words >= 0 && n_words <= kMaxWords, "ebos_evt3_scan: n_words %lld outside [0, 2^30]", (long long)n_words);
  EBOS_REQUIRE(words || n_words == 0, "ebos_evt3_scan: words is NULL");
  EBOS_REQUIRE(((uintptr_t)words & 1) == 0, "ebos_evt3_scan: words is not 2-byte aligned");
  EBOS_REQUIRE(carry_out && totals && scratch, "ebos_evt3_scan: NULL carry_out / totals / scratch");
  EBOS_REQUIRE(((uintptr_t)scratch & 7) == 0, "ebos_evt3_scan: scratch is not 8-byte aligned");
  if (scratch_bytes < scratch_need(n_words)) {
    set_error("ebos_evt3_scan: scratch too small (%zu < %zu)", scratch_bytes, scratch_need(n_words));
    return EBOS_ERR_SCRATCH;
  }
  const int64_t n_chunks = chunks_of(n_words);
  Xf* sums = static_cast<Xf*>(scratch);
  ChunkIn* cin = reinterpret_cast<ChunkIn*>(sums + (n_chunks > 0 ? n_chunks : 1));
  hipStream_t s = as_stream(stream);
  if (n_chunks > 0) {
    hipLaunchKernelGGL(evt3_summary_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, s, words, n_words,
                       (int)(((uintptr_t)words & 15) == 0), sums);
    EBOS_CHECK_LAUNCH("ebos_evt3_scan (summary)");
  }
  hipLaunchKernelGGL(evt3_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, sums, n_chunks, carry_in, carry_out, totals, cin);
  EBOS_CHECK_LAUNCH("ebos_evt3_scan (scan)");
  return EBOS_OK;
}

extern "C" int ebos_evt3_emit(const uint16_t* words, int64_t n_words, const void* scratch, size_t scratch_bytes, int64_t n_events,
                              int64_t n_triggers, int64_t event_capacity, int64_t trigger_capacity, int16_t* x, int16_t* y, int64_t* t,
                              uint8_t* p, int64_t* trig_t, uint8_t* trig_value, uint8_t* trig_id, ebos_stream_t stream) {
  EBOS_REQUIRE(n_words >= 0 && n_words <= kMaxWords, "ebos_evt3_emit: n_words %lld outside [0, 2^30]", (long long)n_words);
  EBOS_REQUIRE(words || n_words == 0, "ebos_evt3_emit: words is NULL");
  EBOS_REQUIRE(((uintptr_t)words & 1) == 0, "ebos_evt3_emit: words is not 2-byte aligned");
  EBOS_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0, "ebos_evt3_emit: scratch is NULL or not 8-byte aligned");
  EBOS_REQUIRE(n_events >= 0 && n_triggers >= 0 && event_capacity >= 0 && trigger_capacity >= 0,
               "ebos_evt3_emit: negative totals or capacities");
  EBOS_REQUIRE(event_capacity >= n_events, "ebos_evt3_emit: event capacity %lld below the slab's %lld events",
               (long long)event_capacity, (long long)n_events);
  EBOS_REQUIRE(trigger_capacity >= n_triggers, "ebos_evt3_emit: trigger capacity %lld below the slab's %lld triggers",
               (long long)trigger_capacity, (long long)n_triggers);
  EBOS_REQUIRE(event_capacity == 0 || (x && y && t && p), "ebos_evt3_emit: NULL event column");
  EBOS_REQUIRE(trigger_capacity == 0 || (trig_t && trig_value && trig_id), "ebos_evt3_emit: NULL trigger column");
  EBOS_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 1) == 0 && (((uintptr_t)t | (uintptr_t)trig_t) & 7) == 0,
               "ebos_evt3_emit: misaligned output column");
  if (scratch_bytes < scratch_need(n_words)) {
    set_error("ebos_evt3_emit: scratch too small (%zu < %zu)", scratch_bytes, scratch_need(n_words));
    return EBOS_ERR_SCRATCH;
  }
  const int64_t n_chunks = chunks_of(n_words);
  if (n_chunks == 0) return EBOS_OK;
  const ChunkIn* cin = reinterpret_cast<const ChunkIn*>(static_cast<const Xf*>(scratch) + n_chunks);
  // (stores are guarded by the totals the caller read, not by the larger capacities: nothing past them is touched)
  hipLaunchKernelGGL(evt3_emit_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, as_stream(stream), words, n_words,
                     (int)(((uintptr_t)words & 15) == 0), cin, (long long)n_events, (long long)n_triggers, x, y, t, p, trig_t, trig_value,
                     trig_id);
  EBOS_CHECK_LAUNCH("ebos_evt3_emit");
  return EBOS_OK;
}
