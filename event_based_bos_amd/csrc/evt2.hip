// evt2.hip -- Prophesee EVT 2.0 and EVT 2.1 word streams and DAT records decoded on the device.  The formats and the entry
// points: include/ebos_hip.h; the state algebra: evt2_core.h; the scans, the stage and the entries' argument checks, shared with
// evt3.hip: word_scan.h; the body of the scan pass, shared as text: word_scan_body.h.
//
// EVT 2.0 / 2.1 carry everything but the time base in the word that emits; the time base (has_th, th, loops) is set by TIME_HIGH
// words.  What a stretch of words does to it, and how much the stretch emits, is a small record that composes (evt2::Xf), so the
// decode is the three-pass scan of evt3.hip over chunks of kChunk words, one 256-thread workgroup per chunk, whole 16-byte loads:
//   1. summary  every thread folds its words into an Xf, the workgroup combines them in order: one Xf per chunk;
//   2. scan     ONE workgroup combines the chunks' records in order from the carried-in state and leaves, per chunk, the incoming
//               state and the exclusive event and trigger offsets (64-bit), plus the slab's totals and the carry-out;
//   3. emit     an exclusive scan of the threads' time records gives every thread the time base before its first word; its output
//               slots come from prefix counts over the wave plus the wave offsets;
//                 EVT 2.0  a compaction, 0 or 1 event a word: ballots; the chunk's events are staged in LDS and stored to their final
//                          places by the whole workgroup, consecutive lanes on consecutive elements;
//                 EVT 2.1  an expansion, 0 to 32 events a word: a lane walks the set bits of its own words into the stage, see
//                          evt21_emit_kernel.
// Integer arithmetic only, no atomics: stream order, the same bytes every run.  Every store is guarded by the caller's totals.
// DAT is fixed records: one streaming kernel.
#include "common.h"
#include "evt2_core.h"
#include "word_scan.h"

namespace ebos {
namespace {

using evt2::Time;
using evt2::Word;
using evt2::Xf;

constexpr int kStage = 2048;  // events the emit pass stages in LDS at a time (13 B each)
using In = ChunkIn<ebos_evt2_state>;

// words per thread: two 16-byte loads of consecutive words
template <int kWordBytes>
struct Format;
template <>
struct Format<4> {
  using word_t = uint32_t;
  static constexpr int kPerThread = 8;
  static constexpr word_t kFiller = 0xF0000000u;  // past the slab's end: an ignored type
  static __device__ __forceinline__ Word classify(word_t w) { return evt2::classify32(w); }
};
template <>
struct Format<8> {
  using word_t = uint64_t;
  static constexpr int kPerThread = 4;
  static constexpr word_t kFiller = 0xF000000000000000ull;
  static __device__ __forceinline__ Word classify(word_t w) { return evt2::classify64(w); }
};
template <int kWordBytes>
constexpr int chunk_of() {
  return kBlock * Format<kWordBytes>::kPerThread;
}
static_assert(chunk_of<4>() <= kStage, "an EVT 2.0 chunk's events fit one stage");

// what a thread's words are to the workgroup scan of the EVT 2.1 emit pass: the time record and the raw event count
struct Lane {
  Time t;
  int ev;
};
__device__ __forceinline__ Lane then(const Lane& u, const Lane& v) { return Lane{evt2::then(u.t, v.t), u.ev + v.ev}; }
using evt2::then;

template <>
__device__ __forceinline__ Time identity_of<Time>() {
  return evt2::time_identity();
}
template <>
__device__ __forceinline__ Xf identity_of<Xf>() {
  return evt2::identity();
}
template <>
__device__ __forceinline__ Lane identity_of<Lane>() {
  return Lane{evt2::time_identity(), 0};
}

// a record through a lane exchange, field by field (f: a value of lane -> the value of another lane)
template <typename F>
__device__ __forceinline__ Time exchange(const Time& x, F f) {
  return Time{f(x.has_th), f(x.first_th), f(x.last_th), f(x.wraps)};
}
template <typename F>
__device__ __forceinline__ Xf exchange(const Xf& x, F f) {
  return Xf{exchange(x.t, f), f(x.ev_a), f(x.tr_a), f(x.ev_b), f(x.tr_b)};
}
template <typename F>
__device__ __forceinline__ Lane exchange(const Lane& x, F f) {
  return Lane{exchange(x.t, f), f(x.ev)};
}

// the thread's words: word k of thread t of chunk c is word c * kChunk + t * kPerThread + k; past the slab's end: an ignored type
template <int kWordBytes>
__device__ __forceinline__ void load_words(const void* __restrict__ words, int64_t n_words, int aligned16, int half_swapped,
                                           typename Format<kWordBytes>::word_t (&w)[Format<kWordBytes>::kPerThread]) {
  using word_t = typename Format<kWordBytes>::word_t;
  constexpr int P = Format<kWordBytes>::kPerThread, kPerLoad = 16 / kWordBytes;
  static_assert(P % kPerLoad == 0, "whole 16-byte loads");
  const word_t* src = static_cast<const word_t*>(words);
  const int64_t base = (int64_t)blockIdx.x * (kBlock * P) + (int64_t)threadIdx.x * P;
  if (aligned16 && base + P <= n_words) {
#pragma unroll
    for (int v = 0; v < P / kPerLoad; ++v) {
      const uint4 q = *reinterpret_cast<const uint4*>(src + base + kPerLoad * v);  // (base is a multiple of P words = 32 B)
      if constexpr (kWordBytes == 4) {
        w[4 * v] = q.x;
        w[4 * v + 1] = q.y;
        w[4 * v + 2] = q.z;
        w[4 * v + 3] = q.w;
      } else {
        w[2 * v] = ((uint64_t)q.y << 32) | q.x;
        w[2 * v + 1] = ((uint64_t)q.w << 32) | q.z;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < P; ++k) w[k] = base + k < n_words ? src[base + k] : Format<kWordBytes>::kFiller;
  }
  if constexpr (kWordBytes == 8) {
    if (half_swapped) {  // (the filler stays what it is)
#pragma unroll
      for (int k = 0; k < P; ++k) w[k] = base + k < n_words ? (w[k] << 32) | (w[k] >> 32) : w[k];
    }
  }
}

template <int kWordBytes>
__global__ __launch_bounds__(kBlock) void evt2_summary_kernel(const void* __restrict__ words, int64_t n_words, int aligned16,
                                                              int half_swapped, Xf* __restrict__ sums) {
  constexpr int P = Format<kWordBytes>::kPerThread;
  __shared__ Xf waves[kWaves];
  typename Format<kWordBytes>::word_t w[P];
  load_words<kWordBytes>(words, n_words, aligned16, half_swapped, w);
  Xf mine = evt2::identity();
#pragma unroll
  for (int k = 0; k < P; ++k) evt2::fold_word(mine, Format<kWordBytes>::classify(w[k]));
  Xf total;
  block_scan_exclusive(mine, waves, total, [](int) {});
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanBlock) void evt2_scan_kernel(const Xf* __restrict__ sums, int64_t n_chunks, const ebos_evt2_state* carry_in,
                                                               ebos_evt2_state* carry_out, int64_t* totals, In* __restrict__ cin) {
  using State = ebos_evt2_state;
#include "word_scan_body.h"
}

// Raw counts and offsets count every event and trigger word, also those before the stream's first TIME_HIGH.  Those are dropped --
// they all come before the first word that counts, so a kept item's number is its raw number minus the dropped ones.
struct Dropped {
  int ev, tr;
};
__device__ __forceinline__ Dropped dropped_of(const In& in, const Xf& sum) {
  return in.s.has_th ? Dropped{0, 0} : Dropped{(int)sum.ev_a, (int)sum.tr_a};
}

// prefix count over the wave of a flag per lane and word: the flags of the lanes before this one, and of the whole wave
template <int P>
__device__ __forceinline__ void ballot_counts(const bool (&flag)[P], int& before, int& wave_total) {
  const unsigned long long below = (1ull << (threadIdx.x & (kWave - 1))) - 1ull;
  before = 0;
  wave_total = 0;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const unsigned long long b = __ballot(flag[k]);
    before += __popcll(b & below);
    wave_total += __popcll(b);
  }
}

__global__ __launch_bounds__(kBlock) void evt2_emit_kernel(const void* __restrict__ words, int64_t n_words, int aligned16,
                                                           const Xf* __restrict__ sums, const In* __restrict__ cin, long long n_events,
                                                           long long n_triggers, int16_t* __restrict__ x, int16_t* __restrict__ y,
                                                           int64_t* __restrict__ t, uint8_t* __restrict__ p, int64_t* __restrict__ trig_t,
                                                           uint8_t* __restrict__ trig_value, uint8_t* __restrict__ trig_id) {
  constexpr int P = Format<4>::kPerThread;
  __shared__ Time wave_time[kWaves];
  __shared__ int wave_ev[kWaves], wave_tr[kWaves];
  __shared__ Stage<kStage> stage;
  uint32_t w[P];
  load_words<4>(words, n_words, aligned16, 0, w);
  // the time record of the thread's own words; its event and trigger words, counted over the wave by ballots
  Time mine = evt2::time_identity();
  bool is_ev[P], is_tr[P];
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int type = (int)(w[k] >> 28);
    is_ev[k] = type <= 1;
    is_tr[k] = type == evt2::kTrigger;
    if (type == evt2::kTimeHigh) mine = then(mine, Time{1, (int)(w[k] & 0x0FFFFFFFu), (int)(w[k] & 0x0FFFFFFFu), 0});
  }
  int ev, ev_wave, tr, tr_wave;
  ballot_counts(is_ev, ev, ev_wave);
  ballot_counts(is_tr, tr, tr_wave);
  Time total;
  const Time pre = block_scan_exclusive(mine, wave_time, total, [&](int wid) {
    wave_ev[wid] = ev_wave;
    wave_tr[wid] = tr_wave;
  });
  const int wid = threadIdx.x / kWave;
#pragma unroll
  for (int v = 0; v < kWaves; ++v) {
    if (v < wid) {
      ev += wave_ev[v];
      tr += wave_tr[v];
    }
  }
  const In in = cin[blockIdx.x];
  const Xf sum = sums[blockIdx.x];
  const Dropped drop = dropped_of(in, sum);
  const int n_ev = (int)(sum.ev_a + sum.ev_b) - drop.ev;  // the chunk's own event count (the same in every thread)
  ebos_evt2_state s = in.s;
  evt2::apply(s, pre);  // the time base before the thread's first word
  ev -= drop.ev;        // (negative only on words that are dropped)
  tr -= drop.tr;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const uint32_t u = w[k];
    const int type = (int)(u >> 28);
    if (type == evt2::kTimeHigh) {
      evt2::step_time_high(s, (int)(u & 0x0FFFFFFFu));
    } else if (is_ev[k]) {
      if (s.has_th && (unsigned)ev < (unsigned)kStage) {  // (0 <= ev < n_ev <= kStage with the scratch of these words)
        stage.x[ev] = (int16_t)((u >> 11) & 0x7FFu);
        stage.y[ev] = (int16_t)(u & 0x7FFu);
        stage.t[ev] = evt2::time_of(s, (int)((u >> 22) & 0x3Fu));
        stage.p[ev] = (uint8_t)type;
      }
      ++ev;
    } else if (is_tr[k]) {
      const long long g = in.tr + tr;
      if (s.has_th && tr >= 0 && g < n_triggers) {
        trig_t[g] = evt2::time_of(s, (int)((u >> 22) & 0x3Fu));
        trig_value[g] = (uint8_t)(u & 1u);
        trig_id[g] = (uint8_t)((u >> 8) & 0x1Fu);
      }
      ++tr;
    }
  }
  __syncthreads();
  store_stage(stage, n_ev < kStage ? n_ev : kStage, in.ev, n_events, x, y, t, p);
}

// EVT 2.1: a word fires 0 to 32 events, a chunk up to 32 kChunk.  Every thread knows the offset of each of its words' first event
// (the workgroup scan of the raw counts) and the word's time; from there a lane walks the set bits of its own words into the LDS
// stage, kStage events a round (a word outside the round is skipped whole), and the workgroup stores the stage.  (A search of every
// output slot for its word was measured against this walk and lost on both kinds of stream: DESIGN 4.36.)
__global__ __launch_bounds__(kBlock) void evt21_emit_kernel(const void* __restrict__ words, int64_t n_words, int aligned16, int half_swapped,
                                                            const Xf* __restrict__ sums, const In* __restrict__ cin,
                                                            long long n_events, long long n_triggers, int16_t* __restrict__ x,
                                                            int16_t* __restrict__ y, int64_t* __restrict__ t, uint8_t* __restrict__ p,
                                                            int64_t* __restrict__ trig_t, uint8_t* __restrict__ trig_value,
                                                            uint8_t* __restrict__ trig_id) {
  constexpr int P = Format<8>::kPerThread;
  __shared__ Lane wave_lane[kWaves];
  __shared__ int wave_tr[kWaves];
  uint64_t w[P];
  load_words<8>(words, n_words, aligned16, half_swapped, w);
  Lane mine = identity_of<Lane>();
  bool is_tr[P];
  int count[P];
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const Word c = evt2::classify64(w[k]);
    is_tr[k] = c.type == evt2::kTrigger;
    count[k] = c.events;
    mine.ev += c.events;
    if (c.type == evt2::kTimeHigh) mine.t = then(mine.t, Time{1, c.th, c.th, 0});
  }
  int tr, tr_wave;
  ballot_counts(is_tr, tr, tr_wave);
  Lane total;
  const Lane pre = block_scan_exclusive(mine, wave_lane, total, [&](int wid) { wave_tr[wid] = tr_wave; });
  const int wid = threadIdx.x / kWave;
#pragma unroll
  for (int v = 0; v < kWaves; ++v) {
    if (v < wid) tr += wave_tr[v];
  }
  const In in = cin[blockIdx.x];
  const Xf sum = sums[blockIdx.x];
  const Dropped drop = dropped_of(in, sum);
  const int n_ev = (int)(sum.ev_a + sum.ev_b) - drop.ev;  // at most 32 kChunk
  ebos_evt2_state s = in.s;
  evt2::apply(s, pre.t);
  tr -= drop.tr;
  // every word's first event number inside the chunk, its time, and whether it counts; the triggers are stored from here
  int off[P];
  long long time[P];
  int ev = pre.ev - drop.ev;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int type = (int)(w[k] >> 60), ts = (int)((w[k] >> 54) & 0x3Full);
    off[k] = ev;
    ev += count[k];
    if (type == evt2::kTimeHigh) evt2::step_time_high(s, (int)((w[k] >> 32) & 0x0FFFFFFFull));
    time[k] = evt2::time_of(s, ts);
    if (!s.has_th) count[k] = 0;  // (a dropped word: off[k] < 0)
    if (is_tr[k]) {
      const long long g = in.tr + tr;
      if (s.has_th && tr >= 0 && g < n_triggers) {
        trig_t[g] = time[k];
        trig_value[g] = (uint8_t)((w[k] >> 32) & 1ull);
        trig_id[g] = (uint8_t)((w[k] >> 40) & 0x1Full);
      }
      ++tr;
    }
  }
  __shared__ Stage<kStage> stage;
  for (int lo = 0; lo < n_ev; lo += kStage) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if (count[k] == 0 || off[k] >= lo + kStage || off[k] + count[k] <= lo) continue;
      const int16_t ey = (int16_t)((w[k] >> 32) & 0x7FFull);
      const int bx = (int)((w[k] >> 43) & 0x7FFull);
      const uint8_t ep = (uint8_t)(w[k] >> 60);
      uint32_t m = (uint32_t)w[k];
      int e = off[k] - lo;
      while (m) {
        const int b = __builtin_ctz(m);
        m &= m - 1;
        if ((unsigned)e < (unsigned)kStage) {
          stage.x[e] = (int16_t)(bx + b);
          stage.y[e] = ey;
          stage.t[e] = time[k];
          stage.p[e] = ep;
        }
        ++e;
      }
    }
    __syncthreads();
    store_stage(stage, n_ev - lo < kStage ? n_ev - lo : kStage, in.ev + lo, n_events, x, y, t, p);
    __syncthreads();
  }
}

// DAT: a lane takes two records in one 16-byte load and stores the pair's x, y, t and p as one store each (kPairs), or one record
// where the caller's pointers do not allow that.
template <bool kPairs>
__global__ __launch_bounds__(kBlock) void dat_decode_kernel(const uint2* __restrict__ records, int64_t n, int version, int16_t* __restrict__ x,
                                                            int16_t* __restrict__ y, int64_t* __restrict__ t, uint8_t* __restrict__ p) {
  const int xbits = version == 1 ? 9 : 14, ybits = version == 1 ? 8 : 14, pshift = version == 1 ? 17 : 28;
  const unsigned xmask = (1u << xbits) - 1u, ymask = (1u << ybits) - 1u;
  const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if constexpr (kPairs) {
    for (int64_t i = first; 2 * i < n; i += stride) {
      if (2 * i + 1 < n) {
        const uint4 q = reinterpret_cast<const uint4*>(records)[i];
        *reinterpret_cast<short2*>(x + 2 * i) = make_short2((short)(q.y & xmask), (short)(q.w & xmask));
        *reinterpret_cast<short2*>(y + 2 * i) = make_short2((short)((q.y >> xbits) & ymask), (short)((q.w >> xbits) & ymask));
        *reinterpret_cast<longlong2*>(t + 2 * i) = make_longlong2((long long)q.x, (long long)q.z);
        *reinterpret_cast<uchar2*>(p + 2 * i) = make_uchar2((unsigned char)((q.y >> pshift) & 1u), (unsigned char)((q.w >> pshift) & 1u));
      } else {  // an odd count's last record
        const uint2 r = records[2 * i];
        x[2 * i] = (int16_t)(r.y & xmask);
        y[2 * i] = (int16_t)((r.y >> xbits) & ymask);
        t[2 * i] = (int64_t)r.x;
        p[2 * i] = (uint8_t)((r.y >> pshift) & 1u);
      }
    }
  } else {
    for (int64_t i = first; i < n; i += stride) {
      const uint2 r = records[i];
      x[i] = (int16_t)(r.y & xmask);
      y[i] = (int16_t)((r.y >> xbits) & ymask);
      t[i] = (int64_t)r.x;
      p[i] = (uint8_t)((r.y >> pshift) & 1u);
    }
  }
}

inline int chunk_words(int word_bytes) { return word_bytes == 4 ? chunk_of<4>() : chunk_of<8>(); }

}  // namespace
}  // namespace ebos

using namespace ebos;

extern "C" int ebos_evt2_chunk_words(int word_bytes) { return word_bytes == 4 || word_bytes == 8 ? chunk_words(word_bytes) : 0; }

extern "C" size_t ebos_evt2_scratch_bytes(int64_t n_words, int word_bytes) {
  if ((word_bytes != 4 && word_bytes != 8) || n_words < 0 || n_words > kMaxWords) return 0;
  return scratch_need<Xf, ebos_evt2_state>(n_words, chunk_words(word_bytes));
}

extern "C" int ebos_evt2_scan(const void* words, int64_t n_words, int word_bytes, int half_swapped, const ebos_evt2_state* carry_in,
                              ebos_evt2_state* carry_out, int64_t* totals, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  EBOS_REQUIRE(word_bytes == 4 || word_bytes == 8, "ebos_evt2_scan: word_bytes %d is neither 4 (EVT 2.0) nor 8 (EVT 2.1)", word_bytes);
  if (const int e = check_scan_args<Xf, ebos_evt2_state>("ebos_evt2_scan", words, n_words, word_bytes, chunk_words(word_bytes), carry_out,
                                                         totals, scratch, scratch_bytes))
    return e;
  const int64_t n_chunks = chunks_of(n_words, chunk_words(word_bytes));
  const auto [sums, cin] = split_scratch<Xf, ebos_evt2_state>(scratch, n_chunks);
  hipStream_t s = as_stream(stream);
  const int aligned16 = (int)(((uintptr_t)words & 15) == 0);
  if (n_chunks > 0) {
    if (word_bytes == 4)
      hipLaunchKernelGGL(evt2_summary_kernel<4>, dim3((unsigned)n_chunks), dim3(kBlock), 0, s, words, n_words, aligned16, 0, sums);
    else
      hipLaunchKernelGGL(evt2_summary_kernel<8>, dim3((unsigned)n_chunks), dim3(kBlock), 0, s, words, n_words, aligned16,
                         half_swapped ? 1 : 0, sums);
    EBOS_CHECK_LAUNCH("ebos_evt2_scan (summary)");
  }
  hipLaunchKernelGGL(evt2_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, sums, n_chunks, carry_in, carry_out, totals, cin);
  EBOS_CHECK_LAUNCH("ebos_evt2_scan (scan)");
  return EBOS_OK;
}

extern "C" int ebos_evt2_emit(const void* words, int64_t n_words, int word_bytes, int half_swapped, const void* scratch, size_t scratch_bytes,
                              int64_t n_events, int64_t n_triggers, int64_t event_capacity, int64_t trigger_capacity, int16_t* x, int16_t* y,
                              int64_t* t, uint8_t* p, int64_t* trig_t, uint8_t* trig_value, uint8_t* trig_id, ebos_stream_t stream) {
  EBOS_REQUIRE(word_bytes == 4 || word_bytes == 8, "ebos_evt2_emit: word_bytes %d is neither 4 (EVT 2.0) nor 8 (EVT 2.1)", word_bytes);
  if (const int e = check_emit_args<Xf, ebos_evt2_state>("ebos_evt2_emit", words, n_words, word_bytes, chunk_words(word_bytes), scratch,
                                                         scratch_bytes, n_events, n_triggers, event_capacity, trigger_capacity, x, y, t, p,
                                                         trig_t, trig_value, trig_id))
    return e;
  const int64_t n_chunks = chunks_of(n_words, chunk_words(word_bytes));
  if (n_chunks == 0) return EBOS_OK;
  const auto [sums, cin] = split_scratch<Xf, ebos_evt2_state>(scratch, n_chunks);
  const int aligned16 = (int)(((uintptr_t)words & 15) == 0);
  const dim3 grid((unsigned)n_chunks), block(kBlock);
  hipStream_t s = as_stream(stream);
  // (stores are guarded by the totals the caller read, not by the larger capacities: nothing past them is touched)
  if (word_bytes == 4)
    hipLaunchKernelGGL(evt2_emit_kernel, grid, block, 0, s, words, n_words, aligned16, sums, cin, (long long)n_events, (long long)n_triggers,
                       x, y, t, p, trig_t, trig_value, trig_id);
  else
    hipLaunchKernelGGL(evt21_emit_kernel, grid, block, 0, s, words, n_words, aligned16, half_swapped ? 1 : 0, sums, cin,
                       (long long)n_events, (long long)n_triggers, x, y, t, p, trig_t, trig_value, trig_id);
  EBOS_CHECK_LAUNCH("ebos_evt2_emit");
  return EBOS_OK;
}

extern "C" int ebos_dat_decode(const void* records, int64_t n_records, int version, int16_t* x, int16_t* y, int64_t* t, uint8_t* p,
                               int64_t capacity, ebos_stream_t stream) {
  EBOS_REQUIRE(n_records >= 0 && n_records <= kMaxWords, "ebos_dat_decode: n_records %lld outside [0, 2^30]", (long long)n_records);
  EBOS_REQUIRE(version == 1 || version == 2, "ebos_dat_decode: version %d is neither 1 nor 2", version);
  EBOS_REQUIRE(capacity >= n_records, "ebos_dat_decode: capacity %lld below the %lld records", (long long)capacity, (long long)n_records);
  EBOS_REQUIRE(records || n_records == 0, "ebos_dat_decode: records is NULL");
  EBOS_REQUIRE(((uintptr_t)records & 7) == 0, "ebos_dat_decode: records is not 8-byte aligned");
  EBOS_REQUIRE(n_records == 0 || (x && y && t && p), "ebos_dat_decode: NULL column");
  EBOS_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 1) == 0 && ((uintptr_t)t & 7) == 0, "ebos_dat_decode: misaligned column");
  if (n_records == 0) return EBOS_OK;
  const bool pairs = ((uintptr_t)records & 15) == 0 && (((uintptr_t)x | (uintptr_t)y) & 3) == 0 && ((uintptr_t)t & 15) == 0 && ((uintptr_t)p & 1) == 0;
  const uint2* rec = static_cast<const uint2*>(records);
  if (pairs)
    hipLaunchKernelGGL(dat_decode_kernel<true>, dim3(stream_grid((n_records + 1) / 2, kBlock)), dim3(kBlock), 0, as_stream(stream), rec,
                       n_records, version, x, y, t, p);
  else
    hipLaunchKernelGGL(dat_decode_kernel<false>, dim3(stream_grid(n_records, kBlock)), dim3(kBlock), 0, as_stream(stream), rec, n_records,
                       version, x, y, t, p);
  EBOS_CHECK_LAUNCH("ebos_dat_decode");
  return EBOS_OK;
}
