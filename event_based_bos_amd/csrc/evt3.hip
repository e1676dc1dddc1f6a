// evt3.hip -- Prophesee EVT 3.0 word streams (the .raw recordings of the reference, src/data_loader/ccs.py:171) decoded on the
// device.  The format and the entry points: include/ebos_hip.h; the state algebra: evt3_core.h; the scans, the stage and the entries'
// argument checks, shared with evt2.hip: word_scan.h; the body of the scan pass, shared as text: word_scan_body.h.
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
#include "word_scan.h"

namespace ebos {
namespace {

using evt3::Xf;

// words per thread, a multiple of 8 (whole 16-byte loads).  16 halves the summary and the scan pass (0.12 + 0.23 against 0.22 + 0.45 ms
// on 64 M words) and doubles the emit pass (1.58 against 0.86 ms: 204 registers a thread)
constexpr int kPerThread = 8;
static_assert(kPerThread % 8 == 0, "whole 16-byte loads");
constexpr int kChunk = kBlock * kPerThread;
constexpr int kStage = 4096;  // events the emit pass stages in LDS at a time (13 B each)
using In = ChunkIn<ebos_evt3_state>;

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
template <>
__device__ __forceinline__ Xf identity_of<Xf>() {
  return evt3::identity();
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
  block_scan_exclusive(fold_words(w), waves, total, [](int) {});
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanBlock) void evt3_scan_kernel(const Xf* __restrict__ sums, int64_t n_chunks, const ebos_evt3_state* carry_in,
                                                               ebos_evt3_state* carry_out, int64_t* totals,
                                                               In* __restrict__ cin) {
  using State = ebos_evt3_state;
#include "word_scan_body.h"
}

// The emit pass's sink: the chunk's events go to the stage (event number `lo` of the chunk onwards); triggers are rare and stored
// directly, in the first stage's walk only.
struct Sink {
  Stage<kStage>* stage;
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
                                                           const In* __restrict__ cin, long long ev_cap, long long tr_cap,
                                                           int16_t* __restrict__ x, int16_t* __restrict__ y, int64_t* __restrict__ t,
                                                           uint8_t* __restrict__ p, int64_t* __restrict__ trig_t,
                                                           uint8_t* __restrict__ trig_value, uint8_t* __restrict__ trig_id) {
  __shared__ Xf waves[kWaves];
  __shared__ Stage<kStage> stage;
  unsigned w[kPerThread];
  load_words(words, n_words, aligned16, w);
  Xf total;
  const Xf pre = block_scan_exclusive(fold_words(w), waves, total, [](int) {});
  const In in = cin[blockIdx.x];
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
    store_stage(stage, n_ev - lo < kStage ? n_ev - lo : kStage, in.ev + lo, ev_cap, x, y, t, p);
    __syncthreads();
  }
}

}  // namespace
}  // namespace ebos

using namespace ebos;

extern "C" int ebos_evt3_chunk_words(void) { return kChunk; }

extern "C" size_t ebos_evt3_scratch_bytes(int64_t n_words) {
  if (n_words < 0 || n_words > kMaxWords) return 0;
  return scratch_need<Xf, ebos_evt3_state>(n_words, kChunk);
}

extern "C" int ebos_evt3_scan(const uint16_t* words, int64_t n_words, const ebos_evt3_state* carry_in, ebos_evt3_state* carry_out,
                              int64_t* totals, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  if (const int e = check_scan_args<Xf, ebos_evt3_state>("ebos_evt3_scan", words, n_words, 2, kChunk, carry_out, totals, scratch, scratch_bytes))
    return e;
  const int64_t n_chunks = chunks_of(n_words, kChunk);
  const auto [sums, cin] = split_scratch<Xf, ebos_evt3_state>(scratch, n_chunks);
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
  if (const int e = check_emit_args<Xf, ebos_evt3_state>("ebos_evt3_emit", words, n_words, 2, kChunk, scratch, scratch_bytes, n_events,
                                                         n_triggers, event_capacity, trigger_capacity, x, y, t, p, trig_t, trig_value, trig_id))
    return e;
  const int64_t n_chunks = chunks_of(n_words, kChunk);
  if (n_chunks == 0) return EBOS_OK;
  const In* cin = split_scratch<Xf, ebos_evt3_state>(scratch, n_chunks).cin;
  // (stores are guarded by the totals the caller read, not by the larger capacities: nothing past them is touched)
  hipLaunchKernelGGL(evt3_emit_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, as_stream(stream), words, n_words,
                     (int)(((uintptr_t)words & 15) == 0), cin, (long long)n_events, (long long)n_triggers, x, y, t, p, trig_t, trig_value,
                     trig_id);
  EBOS_CHECK_LAUNCH("ebos_evt3_emit");
  return EBOS_OK;
}
