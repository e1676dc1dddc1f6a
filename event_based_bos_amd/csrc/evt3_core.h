// evt3_core.h -- the state algebra of the EVT 3.0 decoder (evt3.hip): what a stretch of words does to the decoder's state, as a
// record that composes.  Host and device code: the same functions fold the words of a thread, the threads of a workgroup and the
// chunks of a slab.
//
// The decoder's state is (has_th, th, tl, y, bx, pol, loops) -- include/ebos_hip.h.  A stretch of words splits at its first
// TIME_HIGH:
//   part A, the words before it, acts only on a state that has seen a TIME_HIGH already (every word before the stream's first
//           TIME_HIGH is ignored), and can set tl, y and the vector base and emit events and triggers;
//   part B, from that TIME_HIGH on, always acts: it knows the first and the last TIME_HIGH value and the wraps between them, and its
//           tl is always known (a TIME_HIGH resets tl to 0).
// A part is a `Part`: the last value of each field, or "unset"; the vector base is either absolute (a VECT_BASE_X was seen: bx holds
// its x plus the increments of the vector words after it) or an increment alone.
#pragma once
#include <stdint.h>

#include "ebos_hip.h"

#if defined(__HIPCC__)
#define EVT3_HD __host__ __device__ __forceinline__
#else
#define EVT3_HD inline
#endif

namespace ebos {
namespace evt3 {

struct Part {
  long long ev, tr;  // events and triggers the part emits
  int tl;            // -1: unset
  int y;             // -1: unset
  int base;          // 1: bx is absolute and pol is set; 0: bx is an increment
  int bx;            // modulo 2^16
  int pol;
  int reserved;      // (no padding: a Part is copied as six plain words)
};

struct Xf {
  Part a;
  int has_th, first_th, last_th;
  int wraps;  // wraps between the stretch's own TIME_HIGH words
  Part b;
};

EVT3_HD Part part_identity() { return Part{0, 0, -1, -1, 0, 0, 0, 0}; }
EVT3_HD Xf identity() { return Xf{part_identity(), 0, 0, 0, 0, part_identity()}; }

// the wrap rule of a TIME_HIGH of value v after one of value prev (4096 - 4085 = a threshold of 10 ticks and the value itself)
EVT3_HD int is_wrap(int prev, int v) { return (prev > v && prev - v >= 4085) ? 1 : 0; }

// p, then q
EVT3_HD Part then(const Part& p, const Part& q) {
  Part r;
  r.tl = q.tl >= 0 ? q.tl : p.tl;
  r.y = q.y >= 0 ? q.y : p.y;
  r.base = p.base | q.base;
  r.bx = q.base ? q.bx : ((p.bx + q.bx) & 0xFFFF);
  r.pol = q.base ? q.pol : p.pol;
  r.ev = p.ev + q.ev;
  r.tr = p.tr + q.tr;
  r.reserved = 0;
  return r;
}

// stretch u, then stretch v (associative, not commutative)
EVT3_HD Xf then(const Xf& u, const Xf& v) {
  Xf r;
  if (!u.has_th) {
    r.a = then(u.a, v.a);
    r.has_th = v.has_th;
    r.first_th = v.first_th;
    r.last_th = v.last_th;
    r.wraps = v.wraps;
    r.b = v.b;
    return r;
  }
  r.a = u.a;
  r.has_th = 1;
  r.first_th = u.first_th;
  const Part mid = then(u.b, v.a);
  if (v.has_th) {
    r.last_th = v.last_th;
    r.wraps = u.wraps + is_wrap(u.last_th, v.first_th) + v.wraps;
    r.b = then(mid, v.b);  // (v.b.tl is set: the TIME_HIGH's reset of tl comes with it)
  } else {
    r.last_th = u.last_th;
    r.wraps = u.wraps;
    r.b = mid;
  }
  return r;
}

EVT3_HD void apply(ebos_evt3_state& s, const Part& p) {
  if (p.tl >= 0) s.tl = p.tl;
  if (p.y >= 0) s.y = p.y;
  if (p.base) {
    s.bx = p.bx;
    s.pol = p.pol;
  } else {
    s.bx = (s.bx + p.bx) & 0xFFFF;
  }
}

// the state after a stretch; ev / tr grow by what the stretch emits from that state
EVT3_HD void apply(ebos_evt3_state& s, const Xf& x, long long& ev, long long& tr) {
  if (s.has_th) {
    apply(s, x.a);
    ev += x.a.ev;
    tr += x.a.tr;
  }
  if (x.has_th) {
    s.loops += is_wrap(s.th, x.first_th) + x.wraps;  // (a state without a TIME_HIGH has th = 0: no wrap)
    s.th = x.last_th;
    s.has_th = 1;
    apply(s, x.b);
    ev += x.b.ev;
    tr += x.b.tr;
  }
}

// Folds words one after the other into an Xf: `cur` is the part being written, part A until the first TIME_HIGH.  (Two objects,
// not one: the compiler keeps each in registers.)
EVT3_HD void fold_start(Xf& x, Part& cur) {
  x = identity();
  cur = part_identity();
}
EVT3_HD void fold_word(Xf& x, Part& cur, unsigned w) {
  const int type = (int)(w >> 12) & 0xF, v = (int)(w & 0xFFF);
  if (type == 0x8) {
    if (x.has_th) {
      x.wraps += is_wrap(x.last_th, v);
    } else {
      x.a = cur;
      cur = part_identity();
      x.has_th = 1;
      x.first_th = v;
    }
    x.last_th = v;
    cur.tl = 0;
  } else if (type == 0x6) {
    cur.tl = v;
  } else if (type == 0x0) {
    cur.y = v & 0x7FF;
  } else if (type == 0x2) {
    cur.ev += 1;
  } else if (type == 0x3) {
    cur.base = 1;
    cur.bx = v & 0x7FF;
    cur.pol = v >> 11;
  } else if (type == 0x4) {
    cur.ev += __builtin_popcount((unsigned)v);
    cur.bx = (cur.bx + 12) & 0xFFFF;
  } else if (type == 0x5) {
    cur.ev += __builtin_popcount((unsigned)v & 0xFFu);
    cur.bx = (cur.bx + 8) & 0xFFFF;
  } else if (type == 0xA) {
    cur.tr += 1;
  }
}
EVT3_HD void fold_finish(Xf& x, const Part& cur) {
  if (x.has_th) x.b = cur;
  else x.a = cur;
}

EVT3_HD long long time_of(const ebos_evt3_state& s) { return (s.loops << 24) | ((long long)s.th << 12) | (long long)s.tl; }

// One word on a state, word by word (the emit pass, inside a thread's own words).  Sink: event(x, y, t, p), trigger(t, value, id).
template <typename Sink>
EVT3_HD void step(ebos_evt3_state& s, unsigned w, Sink& out) {
  const int type = (int)(w >> 12) & 0xF, v = (int)(w & 0xFFF);
  if (type == 0x8) {
    s.loops += is_wrap(s.th, v);
    s.th = v;
    s.tl = 0;
    s.has_th = 1;
    return;
  }
  if (!s.has_th) return;
  if (type == 0x6) {
    s.tl = v;
  } else if (type == 0x0) {
    s.y = v & 0x7FF;
  } else if (type == 0x2) {
    out.event(v & 0x7FF, s.y, time_of(s), v >> 11);
  } else if (type == 0x3) {
    s.bx = v & 0x7FF;
    s.pol = v >> 11;
  } else if (type == 0x4 || type == 0x5) {
    const int width = type == 0x4 ? 12 : 8;
    unsigned m = (unsigned)v & ((1u << width) - 1u);
    const long long t = time_of(s);
    while (m) {
      const int b = __builtin_ctz(m);
      m &= m - 1;
      out.event((s.bx + b) & 0xFFFF, s.y, t, s.pol);
    }
    s.bx = (s.bx + width) & 0xFFFF;
  } else if (type == 0xA) {
    out.trigger(time_of(s), v & 1, v >> 8);
  }
}

}  // namespace evt3
}  // namespace ebos
