// evt2_core.h -- the state algebra of the EVT 2.0 / EVT 2.1 decoders (evt2.hip): what a stretch of words does to the decoder's
// state, as a record that composes.  Host and device code (a plain C++ compiler can include this header): the same functions fold
// the words of a thread, the threads of a workgroup and the chunks of a slab.
//
// The decoder's state is (has_th, th, loops) -- include/ebos_hip.h.  Both formats carry everything but the time base inside the
// word that emits, so a stretch of words is
//   Time   what it does to the time base: whether it holds a TIME_HIGH, the first and the last TIME_HIGH value and the wraps
//          between its own TIME_HIGH words;
//   Xf     a Time plus four counts: the events and triggers before its first TIME_HIGH (worth nothing while the incoming state has
//          no time yet: every word before the stream's first TIME_HIGH is ignored) and those from it on.
#pragma once
#include <stdint.h>

#include "ebos_hip.h"

#if defined(__HIPCC__)
#define EVT2_HD __host__ __device__ __forceinline__
#else
#define EVT2_HD inline
#endif

namespace ebos {
namespace evt2 {

constexpr int kTimeHigh = 0x8, kTrigger = 0xA;  // (0x0 / 0x1: an event word of polarity 0 / 1)
constexpr int kWrapFall = (1 << 28) - 11;       // a TIME_HIGH that falls by at least this much is a wrap of the 28-bit value

struct Time {
  int has_th, first_th, last_th;
  int wraps;  // wraps between the stretch's own TIME_HIGH words
};

struct Xf {
  Time t;
  long long ev_a, tr_a;  // events / triggers before the stretch's first TIME_HIGH
  long long ev_b, tr_b;  // from it on
};

EVT2_HD Time time_identity() { return Time{0, 0, 0, 0}; }
EVT2_HD Xf identity() { return Xf{time_identity(), 0, 0, 0, 0}; }

// the wrap rule of a TIME_HIGH of value v after one of value prev
EVT2_HD int is_wrap(int prev, int v) { return (prev > v && prev - v >= kWrapFall) ? 1 : 0; }

// stretch u, then stretch v (associative, not commutative)
EVT2_HD Time then(const Time& u, const Time& v) {
  if (!u.has_th) return v;
  if (!v.has_th) return u;
  return Time{1, u.first_th, v.last_th, u.wraps + is_wrap(u.last_th, v.first_th) + v.wraps};
}

EVT2_HD Xf then(const Xf& u, const Xf& v) {
  Xf r;
  r.t = then(u.t, v.t);
  if (!u.t.has_th) {
    r.ev_a = u.ev_a + v.ev_a;
    r.tr_a = u.tr_a + v.tr_a;
    r.ev_b = v.ev_b;
    r.tr_b = v.tr_b;
  } else {
    r.ev_a = u.ev_a;
    r.tr_a = u.tr_a;
    r.ev_b = u.ev_b + v.ev_a + v.ev_b;
    r.tr_b = u.tr_b + v.tr_a + v.tr_b;
  }
  return r;
}

// the state after a stretch
EVT2_HD void apply(ebos_evt2_state& s, const Time& x) {
  if (!x.has_th) return;
  s.loops += (s.has_th ? is_wrap(s.th, x.first_th) : 0) + x.wraps;
  s.th = x.last_th;
  s.has_th = 1;
}

// the state after a stretch; ev / tr grow by what the stretch emits from that state
EVT2_HD void apply(ebos_evt2_state& s, const Xf& x, long long& ev, long long& tr) {
  if (s.has_th) {
    ev += x.ev_a;
    tr += x.tr_a;
  }
  ev += x.ev_b;  // (zero without a TIME_HIGH)
  tr += x.tr_b;
  apply(s, x.t);
}

// one TIME_HIGH of value v on a state, word by word
EVT2_HD void step_time_high(ebos_evt2_state& s, int v) {
  if (s.has_th) s.loops += is_wrap(s.th, v);
  s.th = v;
  s.has_th = 1;
}

EVT2_HD long long time_of(const ebos_evt2_state& s, int ts) {
  return (long long)((unsigned long long)s.loops << 34) | ((long long)s.th << 6) | (long long)ts;
}

// What one word is, whatever the format: its type, the TIME_HIGH value it carries, and how many events it fires.
struct Word {
  int type, th, events;
};
EVT2_HD Word classify32(uint32_t w) {
  const int type = (int)(w >> 28);
  return Word{type, (int)(w & 0x0FFFFFFFu), type <= 1 ? 1 : 0};
}
EVT2_HD Word classify64(uint64_t w) {
  const int type = (int)(w >> 60);
  return Word{type, (int)((w >> 32) & 0x0FFFFFFFu), type <= 1 ? __builtin_popcount((uint32_t)w) : 0};
}

// folds words one after the other into an Xf, which starts as identity()
EVT2_HD void fold_word(Xf& x, const Word& w) {
  if (w.type == kTimeHigh) {
    if (x.t.has_th) {
      x.t.wraps += is_wrap(x.t.last_th, w.th);
    } else {
      x.t.has_th = 1;
      x.t.first_th = w.th;
    }
    x.t.last_th = w.th;
  } else if (w.type <= 1) {
    if (x.t.has_th) x.ev_b += w.events;
    else x.ev_a += w.events;
  } else if (w.type == kTrigger) {
    if (x.t.has_th) x.tr_b += 1;
    else x.tr_a += 1;
  }
}

}  // namespace evt2
}  // namespace ebos
