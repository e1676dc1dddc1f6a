// word_scan.h -- the skeleton the word-stream decoders share (evt3.hip: EVT 3.0; evt2.hip: EVT 2.0 and EVT 2.1): a decode is a scan
// in three passes over chunks of words, one kBlock-thread workgroup per chunk in the summary and the emit pass and ONE workgroup
// of kScanBlock threads in the scan pass between them.  Here, once:
//   device  a record through a lane exchange, the wave and the workgroup scan of records, the LDS stage of the emit passes and
//           its copy-out; the body of the scan pass is word_scan_body.h, text the two scan kernels include;
//   host    the chunk count, the size and the split of the scratch, and the argument checks of the *_scan and *_emit entries.
// A format brings its algebra along as overloads that argument-dependent lookup finds -- declare them before the first kernel:
//   exchange(x, f)        the record x with f applied to every field (in the including file's namespace ebos::{anonymous});
//   identity_of<T>()      a specialisation per record type;
//   then(u, v)            stretch u, then stretch v (evt3_core.h, evt2_core.h);
//   apply(s, x, ev, tr)   the state after a stretch, ev / tr grown by what it emits from that state (the scan pass only).
// The decoder's start state is the zero-initialised State.
#pragma once
#include "common.h"

namespace ebos {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kScanBlock = 1024;  // the one workgroup of the scan pass
constexpr int64_t kMaxWords = (int64_t)1 << 30;

template <typename State>
struct ChunkIn {
  State s;           // the state before the chunk's first word
  long long ev, tr;  // events / triggers of the slab before the chunk
};

template <typename T>
__device__ __forceinline__ T identity_of();

template <typename T>
__device__ __forceinline__ T shfl_up_rec(const T& x, int off) {
  return exchange(x, [off](auto v) { return __shfl_up(v, off, kWave); });
}
template <typename T>
__device__ __forceinline__ T shfl_rec(const T& x, int lane) {
  return exchange(x, [lane](auto v) { return __shfl(v, lane, kWave); });
}

// inclusive scan of one record per lane over the wave, in lane order
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(const T& mine) {
  const int lane = threadIdx.x & (kWave - 1);
  T inc = mine;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const T o = shfl_up_rec(inc, off);
    if (lane >= off) inc = then(o, inc);
  }
  return inc;
}

// Exclusive scan of one record per thread over the workgroup, in thread order; `total` = all of them.  waves: kWaves records of LDS.
// One barrier: the caller may put values of its own next to the records before it and read them after it (`publish`, lane 63 only);
// a caller that writes waves[] again has to put a barrier of its own in between.
template <typename T, typename Publish>
__device__ __forceinline__ T block_scan_exclusive(const T& mine, T* waves, T& total, Publish publish) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const T inc = wave_scan_inclusive(mine);
  if (lane == kWave - 1) {
    waves[wid] = inc;
    publish(wid);
  }
  __syncthreads();
  T exc = shfl_up_rec(inc, 1);
  if (lane == 0) exc = identity_of<T>();
  T pre = identity_of<T>();
  total = identity_of<T>();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const T t = waves[w];
    if (w < wid) pre = then(pre, t);
    total = then(total, t);
  }
  return then(pre, exc);
}

// The emit passes' stage.  A thread's events are consecutive in the output but few, so stores straight from the threads would touch
// a cache line per lane: the chunk's events go through LDS instead, kStage at a time, and the workgroup copies a full stage out
// with consecutive lanes on consecutive elements.
template <int kStage>
struct Stage {
  int64_t t[kStage];
  int16_t x[kStage];
  int16_t y[kStage];
  uint8_t p[kStage];
};
// the stage's first `count` events to the output's places `first` onwards, below the slab's n_events
template <int kStage>
__device__ __forceinline__ void store_stage(const Stage<kStage>& stage, int count, long long first, long long n_events,
                                            int16_t* __restrict__ x, int16_t* __restrict__ y, int64_t* __restrict__ t,
                                            uint8_t* __restrict__ p) {
  for (int i = threadIdx.x; i < count; i += kBlock) {
    const long long g = first + i;
    if (g < n_events) {
      x[g] = stage.x[i];
      y[g] = stage.y[i];
      t[g] = stage.t[i];
      p[g] = stage.p[i];
    }
  }
}

// ---- host ----------------------------------------------------------------------------------
inline int64_t chunks_of(int64_t n_words, int chunk) { return (n_words + chunk - 1) / chunk; }

// the scratch of a slab: Xf[n] (the summary pass's records), then ChunkIn[n] (what the scan pass leaves), n = max(chunks, 1)
template <typename Xf, typename State>
inline size_t scratch_need(int64_t n_words, int chunk) {
  static_assert(sizeof(Xf) % 8 == 0 && sizeof(ChunkIn<State>) % 8 == 0, "scratch arrays of 8-byte aligned records");
  const int64_t c = chunks_of(n_words, chunk) > 0 ? chunks_of(n_words, chunk) : 1;
  return (size_t)c * (sizeof(Xf) + sizeof(ChunkIn<State>));
}
template <typename Xf, typename State>
struct Scratch {
  Xf* sums;
  ChunkIn<State>* cin;
};
template <typename Xf, typename State>
inline Scratch<Xf, State> split_scratch(const void* scratch, int64_t n_chunks) {
  Xf* sums = static_cast<Xf*>(const_cast<void*>(scratch));  // (the emit entries only read it)
  return {sums, reinterpret_cast<ChunkIn<State>*>(sums + (n_chunks > 0 ? n_chunks : 1))};
}

// The argument checks of an entry `name` = ebos_*_scan / ebos_*_emit, words of word_bytes bytes in chunks of `chunk`: EBOS_OK, or
// the entry's return value with the error set.
inline int check_words(const char* name, const void* words, int64_t n_words, int word_bytes) {
  EBOS_REQUIRE(n_words >= 0 && n_words <= kMaxWords, "%s: n_words %lld outside [0, 2^30]", name, (long long)n_words);
  EBOS_REQUIRE(words || n_words == 0, "%s: words is NULL", name);
  EBOS_REQUIRE(((uintptr_t)words & (uintptr_t)(word_bytes - 1)) == 0, "%s: words is not %d-byte aligned", name, word_bytes);
  return EBOS_OK;
}
template <typename Xf, typename State>
inline int check_scratch_size(const char* name, int64_t n_words, int chunk, size_t scratch_bytes) {
  const size_t need = scratch_need<Xf, State>(n_words, chunk);
  if (scratch_bytes < need) {
    set_error("%s: scratch too small (%zu < %zu)", name, scratch_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  return EBOS_OK;
}
template <typename Xf, typename State>
inline int check_scan_args(const char* name, const void* words, int64_t n_words, int word_bytes, int chunk, const void* carry_out,
                           const void* totals, const void* scratch, size_t scratch_bytes) {
  if (const int e = check_words(name, words, n_words, word_bytes)) return e;
  EBOS_REQUIRE(carry_out && totals && scratch, "%s: NULL carry_out / totals / scratch", name);
  EBOS_REQUIRE(((uintptr_t)scratch & 7) == 0, "%s: scratch is not 8-byte aligned", name);
  return check_scratch_size<Xf, State>(name, n_words, chunk, scratch_bytes);
}
template <typename Xf, typename State>
inline int check_emit_args(const char* name, const void* words, int64_t n_words, int word_bytes, int chunk, const void* scratch,
                           size_t scratch_bytes, int64_t n_events, int64_t n_triggers, int64_t event_capacity, int64_t trigger_capacity,
                           const int16_t* x, const int16_t* y, const int64_t* t, const uint8_t* p, const int64_t* trig_t,
                           const uint8_t* trig_value, const uint8_t* trig_id) {
  if (const int e = check_words(name, words, n_words, word_bytes)) return e;
  EBOS_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0, "%s: scratch is NULL or not 8-byte aligned", name);
  EBOS_REQUIRE(n_events >= 0 && n_triggers >= 0 && event_capacity >= 0 && trigger_capacity >= 0, "%s: negative totals or capacities",
               name);
  EBOS_REQUIRE(event_capacity >= n_events, "%s: event capacity %lld below the slab's %lld events", name, (long long)event_capacity,
               (long long)n_events);
  EBOS_REQUIRE(trigger_capacity >= n_triggers, "%s: trigger capacity %lld below the slab's %lld triggers", name,
               (long long)trigger_capacity, (long long)n_triggers);
  EBOS_REQUIRE(event_capacity == 0 || (x && y && t && p), "%s: NULL event column", name);
  EBOS_REQUIRE(trigger_capacity == 0 || (trig_t && trig_value && trig_id), "%s: NULL trigger column", name);
  EBOS_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 1) == 0 && (((uintptr_t)t | (uintptr_t)trig_t) & 7) == 0,
               "%s: misaligned output column", name);
  return check_scratch_size<Xf, State>(name, n_words, chunk, scratch_bytes);
}

}  // namespace
}  // namespace ebos
