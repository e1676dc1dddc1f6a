// flow_voxel_adjoint.h -- one pixel of the adjoint of one advection step of flow_voxel.hip, and the derivative rules it rests on.
//
// The step is  out = sign * S(sign * in);  its adjoint  d in = J_S(f)^T d out  with f = sign * in  needs no sign of its own: every
// branch decision (max0, min0, sign_of) is taken from f, the values the forward took them from.  The rules are torch's:
//   maximum(x, 0) and minimum(x, 0) pass half the gradient each where x == 0 (and all of it where x is NaN),
//   sign() has no gradient, x ** 2 passes 2 x, (-x) * x passes -2 x.
// A pixel gathers: it reads the upstream gradient at itself and its four neighbours, nothing is scattered.
//
// Plain templates without device-only calls, so a host build can check them against autograd.
#pragma once

#ifndef EBOS_HD
#define EBOS_HD __host__ __device__ __forceinline__
#endif

namespace ebos {
namespace flow_adjoint {

template <typename T>
EBOS_HD T max0(T x) { return x > T(0) ? x : (x != x ? x : T(0)); }
template <typename T>
EBOS_HD T min0(T x) { return x < T(0) ? x : (x != x ? x : T(0)); }
template <typename T>
EBOS_HD T sign_of(T x) { return x > T(0) ? T(1) : (x < T(0) ? T(-1) : (x != x ? x : T(0))); }
// d maximum(x, 0) / dx and d minimum(x, 0) / dx
template <typename T>
EBOS_HD T d_max0(T x) { return x < T(0) ? T(0) : (x == T(0) ? T(0.5) : T(1)); }
template <typename T>
EBOS_HD T d_min0(T x) { return x > T(0) ? T(0) : (x == T(0) ? T(0.5) : T(1)); }

template <typename T>
struct StepGeometry {
  int scheme;   // EBOS_FLOW_UPWIND | EBOS_FLOW_BURGERS
  int H, W;
  T dt;         // |dt|
  T dx, dy;
};

// F(c, i, j): component c of the sign-swapped input flow of the step; G(c, i, j): the gradient of the step's (sign-swapped ... the
// signs cancel) output.  Both are asked for pixels of the image only, (i, j) and its four neighbours.  -> the gradient of the
// step's input at (i, j).
template <typename T, typename Flow, typename Grad>
EBOS_HD void step_adjoint_pixel(const StepGeometry<T>& s, Flow F, Grad G, int i, int j, T* d_u, T* d_v) {
  const bool up = i > 0, down = i + 1 < s.H, left = j > 0, right = j + 1 < s.W;
  const T u = F(0, i, j), v = F(1, i, j);
  const T gu = G(0, i, j), gv = G(1, i, j);
  const T hu = -s.dt * gu, hv = -s.dt * gv;   // the gradients of the two bracketed sums at this pixel
  const T up0 = max0(u), un0 = min0(u), vp0 = max0(v), vn0 = min0(v);
  // the same at the neighbours, 0 where there is none
  const T hu_n = up ? -s.dt * G(0, i - 1, j) : T(0), hu_s = down ? -s.dt * G(0, i + 1, j) : T(0);
  const T hu_w = left ? -s.dt * G(0, i, j - 1) : T(0), hu_e = right ? -s.dt * G(0, i, j + 1) : T(0);
  const T hv_n = up ? -s.dt * G(1, i - 1, j) : T(0), hv_s = down ? -s.dt * G(1, i + 1, j) : T(0);
  const T hv_w = left ? -s.dt * G(1, i, j - 1) : T(0), hv_e = right ? -s.dt * G(1, i, j + 1) : T(0);
  if (s.scheme == EBOS_FLOW_UPWIND) {
    const T u_n = up ? F(0, i - 1, j) : T(0), u_s = down ? F(0, i + 1, j) : T(0);
    const T u_w = left ? F(0, i, j - 1) : T(0), u_e = right ? F(0, i, j + 1) : T(0);
    const T v_n = up ? F(1, i - 1, j) : T(0), v_s = down ? F(1, i + 1, j) : T(0);
    const T v_w = left ? F(1, i, j - 1) : T(0), v_e = right ? F(1, i, j + 1) : T(0);
    const T u_dx_back = (up ? u - u_n : T(0)) / s.dx, u_dx_forw = (down ? u_s - u : T(0)) / s.dx;
    const T u_dy_back = (left ? u - u_w : T(0)) / s.dx, u_dy_forw = (right ? u_e - u : T(0)) / s.dx;
    const T v_dx_back = (up ? v - v_n : T(0)) / s.dy, v_dx_forw = (down ? v_s - v : T(0)) / s.dy;
    const T v_dy_back = (left ? v - v_w : T(0)) / s.dy, v_dy_forw = (right ? v_e - v : T(0)) / s.dy;
    // the coefficients of this pixel's own differences
    const T own = (((up ? up0 : T(0)) - (down ? un0 : T(0))) + (left ? vp0 : T(0))) - (right ? vn0 : T(0));
    // through max0 / min0 of this pixel, its own differences, and the differences of the four neighbours that hold this pixel
    T du = gu + d_max0(u) * (hu * u_dx_back + hv * v_dx_back) + d_min0(u) * (hu * u_dx_forw + hv * v_dx_forw);
    du += hu * own / s.dx;
    du += (((hu_n * min0(u_n) - hu_s * max0(u_s)) + hu_w * min0(v_w)) - hu_e * max0(v_e)) / s.dx;
    T dv = gv + d_max0(v) * (hu * u_dy_back + hv * v_dy_back) + d_min0(v) * (hu * u_dy_forw + hv * v_dy_forw);
    dv += hv * own / s.dy;
    dv += (((hv_n * min0(u_n) - hv_s * max0(u_s)) + hv_w * min0(v_w)) - hv_e * max0(v_e)) / s.dy;
    *d_u = du;
    *d_v = dv;
  } else {
    const T u_w = left ? F(0, i, j - 1) : T(0), u_e = right ? F(0, i, j + 1) : T(0);
    const T v_n = up ? F(1, i - 1, j) : T(0), v_s = down ? F(1, i + 1, j) : T(0);
    const T u_n = up ? F(0, i - 1, j) : T(0), u_s = down ? F(0, i + 1, j) : T(0);
    const T v_w = left ? F(1, i, j - 1) : T(0), v_e = right ? F(1, i, j + 1) : T(0);
    const T u_dy_back = (left ? u - u_w : T(0)) / s.dx, u_dy_forw = (right ? u_e - u : T(0)) / s.dx;
    const T v_dx_back = (up ? v - v_n : T(0)) / s.dy, v_dx_forw = (down ? v_s - v : T(0)) / s.dy;
    // the conservative terms: this pixel is the "back" value of the pixel after it and, on the first row / column, of itself; the
    // "forw" value of the pixel before it and, on the last row / column, of itself (replicated edges)
    const T hu_as_back = hu_s + (up ? T(0) : hu), hu_as_forw = hu_n + (down ? T(0) : hu);
    const T hv_as_back = hv_e + (left ? T(0) : hv), hv_as_forw = hv_w + (right ? T(0) : hv);
    T du = gu + d_max0(u) * (hv * v_dx_back) + d_min0(u) * (hv * v_dx_forw);
    du += hu * ((left ? vp0 : T(0)) - (right ? vn0 : T(0))) / s.dx;
    du += (hu_w * min0(v_w) - hu_e * max0(v_e)) / s.dx;
    du += (hu * (u * sign_of(u)) - hu_as_back * (max0(sign_of(u)) * u)) - hu_as_forw * (min0(sign_of(u)) * u);
    T dv = gv + d_max0(v) * (hu * u_dy_back) + d_min0(v) * (hu * u_dy_forw);
    dv += hv * ((up ? up0 : T(0)) - (down ? un0 : T(0))) / s.dy;
    dv += (hv_n * min0(u_n) - hv_s * max0(u_s)) / s.dy;
    dv += (hv * (v * sign_of(v)) - hv_as_back * (max0(sign_of(v)) * v)) - hv_as_forw * (min0(sign_of(v)) * v);
    *d_u = du;
    *d_v = dv;
  }
}

// torch.clamp(x, -c, c) passes the gradient where -c <= x <= c, bounds included
template <typename T>
EBOS_HD T clamp_pass(T x, int has_clamp, T c) { return (!has_clamp || (-c <= x && x <= c)) ? T(1) : T(0); }

}  // namespace flow_adjoint
}  // namespace ebos
