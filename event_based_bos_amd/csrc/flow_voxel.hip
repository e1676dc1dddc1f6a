// flow_voxel.hip -- the time-aware flow of the reference's utils (src/utils/flow_utils.py): one dense flow at t0 becomes a flow per
// time bin.
//
//   upwind_flow_to_voxel (:447-499)              one first-order upwind step of  F_t + (F . grad) F = 0
//   inviscid_burger_flow_to_voxel (:559-627)     the same with the conservative (Burgers) form of u u_x and v v_y
//   construct_dense_flow_voxel (:97-224)         bin t0 is the input, the bins below it repeated steps with -1/T, above it with +1/T
//   propagate_flow_to_voxel "bilinear" (:243-294) every pixel votes its flow into the four neighbours of (x + u dt, y + v dt)
//   truncate_voxel_flow "mean" (:85-90)          the masked mean over the bins
//
// x is the row direction (flow[0] moves along H), y the column direction.  Every product, sum, difference and quotient is rounded on
// its own (fp contract off for the whole file) and in the reference's order, so a step is the reference's step bit for bit and a chain
// of steps is too.  A step with dt < 0 is the step of the negated flow, negated (:464-467): the chain below t0 carries the negated
// flow and negates what it stores, which is the same bits.
//
// The chain kernel keeps a 32 x 32 tile and a halo of k pixels (k = the steps of its direction, at most kHaloCap) in LDS, runs the k
// steps there -- step s on the tile grown by k - s pixels, so every value a later step reads is the value the whole-image step has
// there: the same expression on the same inputs -- and stores each bin's interior.  Longer chains take one launch per step through the
// bins themselves; a clamp is then a launch of its own at the end, because the reference clamps the finished voxel, not the steps.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace ebos {
namespace {

constexpr int kBlock = 256;
constexpr int kTile = 32;
constexpr int kHaloCap = EBOS_FLOW_VOXEL_HALO_CAP;
constexpr int kRegion = kTile + 2 * kHaloCap;                                  // 48: the tile with its largest halo
constexpr int kGrown = kTile + 2 * (kHaloCap - 1);                             // 46: the widest square a step updates
constexpr int kCells = (kGrown * kGrown + kBlock - 1) / kBlock;                // 9 cells per lane at most
static_assert(sizeof(double) * 2 * kRegion * kRegion <= 64 * 1024, "the tile with its halo has to fit the workgroup's LDS");

// np.maximum(x, 0) / np.minimum(x, 0): NaN comes through (fmax would drop it)
template <typename T>
__device__ __forceinline__ T max0(T x) { return x > T(0) ? x : (x != x ? x : T(0)); }
template <typename T>
__device__ __forceinline__ T min0(T x) { return x < T(0) ? x : (x != x ? x : T(0)); }
template <typename T>
__device__ __forceinline__ T sign_of(T x) { return x > T(0) ? T(1) : (x < T(0) ? T(-1) : (x != x ? x : T(0))); }
// np.clip / torch.clamp with bounds (-c, c): min(max(x, -c), c), NaN comes through
template <typename T>
__device__ __forceinline__ T clamp_to(T x, T c) {
  if (x != x) return x;
  const T lo = -c;
  x = x > lo ? x : lo;
  return x < c ? x : c;
}

template <typename T>
struct Step {
  int scheme;   // EBOS_FLOW_UPWIND | EBOS_FLOW_BURGERS
  int H, W;
  T dt;         // |dt|
  T dx, dy;
};

// One pixel of one step.  at(c, i, j): component c of the (sign-swapped) flow at row i, column j; only pixels of the image are asked for.
template <typename T, typename At>
__device__ __forceinline__ void step_pixel(const Step<T>& s, At at, int i, int j, T* out_u, T* out_v) {
  const T u = at(0, i, j), v = at(1, i, j);
  const bool up = i > 0, down = i + 1 < s.H, left = j > 0, right = j + 1 < s.W;
  if (s.scheme == EBOS_FLOW_UPWIND) {
    // np.diff padded with one zero, then divided: u_dy by dx and v_dx by dy, as the reference has it (:479-486)
    const T u_dx_back = (up ? u - at(0, i - 1, j) : T(0)) / s.dx, u_dx_forw = (down ? at(0, i + 1, j) - u : T(0)) / s.dx;
    const T u_dy_back = (left ? u - at(0, i, j - 1) : T(0)) / s.dx, u_dy_forw = (right ? at(0, i, j + 1) - u : T(0)) / s.dx;
    const T v_dx_back = (up ? v - at(1, i - 1, j) : T(0)) / s.dy, v_dx_forw = (down ? at(1, i + 1, j) - v : T(0)) / s.dy;
    const T v_dy_back = (left ? v - at(1, i, j - 1) : T(0)) / s.dy, v_dy_forw = (right ? at(1, i, j + 1) - v : T(0)) / s.dy;
    const T up0 = max0(u), un0 = min0(u), vp0 = max0(v), vn0 = min0(v);
    *out_u = u - s.dt * (((up0 * u_dx_back + un0 * u_dx_forw) + vp0 * u_dy_back) + vn0 * u_dy_forw);
    *out_v = v - s.dt * (((up0 * v_dx_back + un0 * v_dx_forw) + vp0 * v_dy_back) + vn0 * v_dy_forw);
  } else {
    // replicated edges for the conservative terms (:590-593), zero-padded differences for the cross terms (:611-617)
    const T u_forw = at(0, down ? i + 1 : i, j), u_back = at(0, up ? i - 1 : i, j);
    const T v_forw = at(1, i, right ? j + 1 : j), v_back = at(1, i, left ? j - 1 : j);
    const T bf_u = (((u * u) * sign_of(u) + max0(sign_of(u_back)) * ((-u_back) * u_back)) - min0(sign_of(u_forw)) * (u_forw * u_forw)) / T(2);
    const T bf_v = (((v * v) * sign_of(v) + max0(sign_of(v_back)) * ((-v_back) * v_back)) - min0(sign_of(v_forw)) * (v_forw * v_forw)) / T(2);
    const T u_dy_back = (left ? u - at(0, i, j - 1) : T(0)) / s.dx, u_dy_forw = (right ? at(0, i, j + 1) - u : T(0)) / s.dx;
    const T v_dx_back = (up ? v - at(1, i - 1, j) : T(0)) / s.dy, v_dx_forw = (down ? at(1, i + 1, j) - v : T(0)) / s.dy;
    const T up0 = max0(u), un0 = min0(u), vp0 = max0(v), vn0 = min0(v);
    const T zero = T(0);   // the reference multiplies by arrays of zeros (:621-624): NaN and Inf stay NaN
    *out_u = u - s.dt * ((((up0 * zero + un0 * zero) + vp0 * u_dy_back) + vn0 * u_dy_forw) + bf_u);
    *out_v = v - s.dt * ((((up0 * v_dx_back + un0 * v_dx_forw) + vp0 * zero) + vn0 * zero) + bf_v);
  }
}

// ---------------------------------------------------------------------------------------------------- one launch per step
// out[b] = sign * step(sign * in[b]); in / out [.., 2, H, W] with batch strides of their own (a bin of the voxel, or a flow)
template <typename T>
__global__ __launch_bounds__(kBlock) void step_kernel(Step<T> s, T sign, const T* __restrict__ in, int64_t in_bs, T* __restrict__ out,
                                                      int64_t out_bs) {
  const int64_t plane = (int64_t)s.H * s.W;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= plane) return;
  const int i = (int)(p / s.W), j = (int)(p % s.W);
  const T* src = in + (int64_t)blockIdx.y * in_bs;
  auto at = [&](int c, int ii, int jj) { return src[c * plane + (int64_t)ii * s.W + jj] * sign; };
  T nu, nv;
  step_pixel(s, at, i, j, &nu, &nv);
  T* dst = out + (int64_t)blockIdx.y * out_bs;
  dst[p] = nu * sign;
  dst[plane + p] = nv * sign;
}

// out[b, t] = clamp(in[b]) for every bin: scheme "same", and bin t0 of the per-step route (n_bins = 1, unclamped)
template <typename T>
__global__ __launch_bounds__(kBlock) void broadcast_kernel(const T* __restrict__ in, int64_t n, int n_bins, int64_t out_bs, int has_clamp,
                                                           T clamp, T* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  T v = in[(int64_t)blockIdx.y * n + p];
  if (has_clamp) v = clamp_to(v, clamp);
  T* dst = out + (int64_t)blockIdx.y * out_bs + p;
  for (int t = 0; t < n_bins; ++t) dst[(int64_t)t * n] = v;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void clamp_kernel(T* __restrict__ data, int64_t n, T clamp) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) data[p] = clamp_to(data[p], clamp);
}

// ---------------------------------------------------------------------------------------------------- the chain in LDS
struct Chain {
  int B, T, t0;
  int k_back, k_forw;   // steps below and above t0, each <= kHaloCap
  int wrap_bin;         // >= 0: the bin the last backward step goes to instead of bin -1 (the torch Burgers constructor); else -1
  int write_t0;         // the forward workgroup stores the input as bin t0
  int has_clamp;
};

// grid (tiles along W, tiles along H, 2 B): z = 2 b + direction, direction 0 above t0 (and bin t0 itself), 1 below
template <typename T>
__global__ __launch_bounds__(kBlock) void chain_kernel(Step<T> s, Chain c, T clamp, const T* __restrict__ in, T* __restrict__ out) {
  __shared__ T tile[2][kRegion][kRegion];
  const int b = blockIdx.z >> 1, dir = blockIdx.z & 1;
  const int k = dir ? c.k_back : c.k_forw;
  if (k == 0 && (dir || !c.write_t0)) return;
  const T sign = dir ? T(-1) : T(1);
  const int H = s.H, W = s.W;
  const int64_t plane = (int64_t)H * W;
  const int i0 = blockIdx.y * kTile - k, j0 = blockIdx.x * kTile - k;   // image position of tile[.][0][0]
  const int R = kTile + 2 * k;
  const T* src = in + (int64_t)b * 2 * plane;
  T* dst = out + (int64_t)b * c.T * 2 * plane;

  for (int n = threadIdx.x; n < R * R; n += kBlock) {
    const int ri = n / R, rj = n % R, i = i0 + ri, j = j0 + rj;
    if (i < 0 || i >= H || j < 0 || j >= W) continue;                   // (never read: a step asks for pixels of the image only)
    const T u = src[(int64_t)i * W + j], v = src[plane + (int64_t)i * W + j];
    tile[0][ri][rj] = u * sign;
    tile[1][ri][rj] = v * sign;
    if (!dir && c.write_t0 && ri >= k && ri < k + kTile && rj >= k && rj < k + kTile) {
      T* o = dst + (int64_t)c.t0 * 2 * plane + (int64_t)i * W + j;
      o[0] = c.has_clamp ? clamp_to(u, clamp) : u;
      o[plane] = c.has_clamp ? clamp_to(v, clamp) : v;
    }
  }
  __syncthreads();

  auto at = [&](int comp, int i, int j) { return tile[comp][i - i0][j - j0]; };
  for (int step = 1; step <= k; ++step) {
    int bin = dir ? c.t0 - step : c.t0 + step;
    if (bin < 0) bin = c.wrap_bin;
    const int wa = R - 2 * step;                                         // the tile grown by k - step pixels
    T nu[kCells], nv[kCells];
#pragma unroll
    for (int q = 0; q < kCells; ++q) {
      const int n = threadIdx.x + q * kBlock;
      if (n >= wa * wa) continue;
      const int ri = step + n / wa, rj = step + n % wa, i = i0 + ri, j = j0 + rj;
      if (i < 0 || i >= H || j < 0 || j >= W) continue;
      step_pixel(s, at, i, j, &nu[q], &nv[q]);
      if (ri >= k && ri < k + kTile && rj >= k && rj < k + kTile) {
        T* o = dst + (int64_t)bin * 2 * plane + (int64_t)i * W + j;
        const T ou = nu[q] * sign, ov = nv[q] * sign;
        o[0] = c.has_clamp ? clamp_to(ou, clamp) : ou;
        o[plane] = c.has_clamp ? clamp_to(ov, clamp) : ov;
      }
    }
    __syncthreads();
    if (step == k) break;
#pragma unroll
    for (int q = 0; q < kCells; ++q) {
      const int n = threadIdx.x + q * kBlock;
      if (n >= wa * wa) continue;
      const int ri = step + n / wa, rj = step + n % wa, i = i0 + ri, j = j0 + rj;
      if (i < 0 || i >= H || j < 0 || j >= W) continue;
      tile[0][ri][rj] = nu[q];
      tile[1][ri][rj] = nv[q];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------- bilinear propagation
// grid (pixels, B * n_bins).  The reference's four taps (:258-284): cells (x1, y1), (x1 + 1, y1), (x1, y1 + 1), (x1 + 1, y1 + 1) with
// the weights (1 - fx)(1 - fy), (1 - fx) fy, fx (1 - fy), fx fy IN THAT ORDER -- the second and third are swapped against the cells,
// as in the reference.  A tap outside the image adds value * 0 to cell 0 (:288-292): nothing, unless the value is not finite.
template <typename T>
__global__ __launch_bounds__(kBlock) void bilinear_kernel(const T* __restrict__ in, int H, int W, int n_bins, int t_off, int denom, double dt_single,
                                                          T* __restrict__ out) {
  const int64_t plane = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.y / n_bins, t = blockIdx.y % n_bins;
  const T dt = (T)(denom > 0 ? (double)(t - t_off) / (double)denom : dt_single);
  const int i = (int)(p / W), j = (int)(p % W);
  const T* src = in + (int64_t)b * 2 * plane;
  T* dst = out + ((int64_t)b * n_bins + t) * 2 * plane;
  const T f0 = src[p], f1 = src[plane + p];
  const T x = f0 * dt + (T)i, y = f1 * dt + (T)j;
  const T x1 = floor(x + (T)1e-8), y1 = floor(y + (T)1e-8);
  const T fx = x - x1, fy = y - y1;
  const T w[4] = {(T(1) - fx) * (T(1) - fy), (T(1) - fx) * fy, fx * (T(1) - fy), fx * fy};
  const T cx[4] = {x1, x1 + T(1), x1, x1 + T(1)}, cy[4] = {y1, y1, y1 + T(1), y1 + T(1)};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool inside = T(0) <= cy[q] && cy[q] < (T)W && T(0) <= cx[q] && cx[q] < (T)H;
    const int64_t cell = inside ? (int64_t)cx[q] * W + (int64_t)cy[q] : 0;
    const T m = inside ? T(1) : T(0);
    const T a0 = (w[q] * f0) * m, a1 = (w[q] * f1) * m;
    if (a0 != T(0)) atomic_add(dst + cell, a0);
    if (a1 != T(0)) atomic_add(dst + plane + cell, a1);
  }
}

// ---------------------------------------------------------------------------------------------------- truncate
// [T, 2, H, W] -> [2, H, W] double: sum_t(flow * mask) / (sum_t(mask) + 1e-6), mask = |flow| > 0 (:85-90), bins in index order
template <typename T>
__global__ __launch_bounds__(kBlock) void truncate_kernel(const T* __restrict__ voxel, int n_bins, int64_t plane, double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= plane) return;
  T su = T(0), sv = T(0);
  long long count = 0;
  for (int t = 0; t < n_bins; ++t) {
    const T u = voxel[((int64_t)t * 2) * plane + p], v = voxel[((int64_t)t * 2 + 1) * plane + p];
    const bool m = u * u + v * v > T(0);   // sqrt(u u + v v) > 0
    const T mf = m ? T(1) : T(0);
    su = t == 0 ? u * mf : su + u * mf;
    sv = t == 0 ? v * mf : sv + v * mf;
    count += m ? 1 : 0;
  }
  const double den = (double)count + 1e-6;
  out[p] = (double)su / den;
  out[plane + p] = (double)sv / den;
}

// ---------------------------------------------------------------------------------------------------- hosts
template <typename T>
int check_step(const char* who, int B, int H, int W, const void* in, const void* out, double dt, double dx, double dy) {
  EBOS_REQUIRE(B > 0 && B <= 32767 && H > 0 && W > 0, "%s: %d flows of %d x %d (1 .. 32767 flows)", who, B, H, W);
  EBOS_REQUIRE((int64_t)H * W <= 2147483647ll, "%s: %d x %d pixels", who, H, W);
  EBOS_REQUIRE(in && out, "%s: NULL buffer", who);
  EBOS_REQUIRE(dt == dt && dx == dx && dy == dy, "%s: dt, dx and dy must be numbers", who);
  return EBOS_OK;
}

// [a, a + na) and [b, b + nb) elements of T share no byte
template <typename T>
bool disjoint(const T* a, int64_t na, const T* b, int64_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 + sizeof(T) * (uint64_t)na <= b0 || b0 + sizeof(T) * (uint64_t)nb <= a0;
}

template <typename T>
Step<T> make_step(int scheme, int H, int W, double dt, double dx, double dy) {
  Step<T> s;
  s.scheme = scheme; s.H = H; s.W = W;
  s.dt = (T)fabs(dt); s.dx = (T)dx; s.dy = (T)dy;
  return s;
}

template <typename T>
int single_step(const char* who, int scheme, int B, int H, int W, const T* in, T* out, double dt, double dx, double dy, ebos_stream_t stream) {
  if (int rc = check_step<T>(who, B, H, W, in, out, dt, dx, dy)) return rc;
  EBOS_REQUIRE(dt != 0.0, "%s: dt = 0 is the identity, there is nothing to launch", who);
  const int64_t plane = (int64_t)H * W;
  EBOS_REQUIRE(disjoint(in, (int64_t)B * 2 * plane, static_cast<const T*>(out), (int64_t)B * 2 * plane), "%s: out overlaps the flow; a step cannot run in place", who);
  hipLaunchKernelGGL(step_kernel<T>, dim3((unsigned)((plane + kBlock - 1) / kBlock), B), dim3(kBlock), 0, as_stream(stream),
                     make_step<T>(scheme, H, W, dt, dx, dy), dt < 0.0 ? T(-1) : T(1), in, 2 * plane, out, 2 * plane);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

template <typename T>
int advect(const char* who, int scheme, int B, int n_bins, int H, int W, const T* in, T* out, int t0, int has_clamp, double clamp,
           int wrap_last, int route, ebos_stream_t stream) {
  if (int rc = check_step<T>(who, B, H, W, in, out, 1.0, 1.0, 1.0)) return rc;
  EBOS_REQUIRE(scheme == EBOS_FLOW_UPWIND || scheme == EBOS_FLOW_BURGERS || scheme == EBOS_FLOW_SAME, "%s: unknown scheme %d", who, scheme);
  EBOS_REQUIRE(n_bins > 0 && t0 >= 0 && t0 < n_bins, "%s: bin %d of %d", who, t0, n_bins);
  EBOS_REQUIRE(route >= EBOS_FLOW_ROUTE_AUTO && route <= EBOS_FLOW_ROUTE_STEPS, "%s: unknown route %d", who, route);
  EBOS_REQUIRE(!has_clamp || clamp == clamp, "%s: the clamp must be a number", who);
  const hipStream_t st = as_stream(stream);
  const int64_t plane = (int64_t)H * W, flow = 2 * plane, voxel = (int64_t)n_bins * flow;
  EBOS_REQUIRE(disjoint(in, (int64_t)B * flow, static_cast<const T*>(out), (int64_t)B * voxel), "%s: out overlaps the flows", who);
  const unsigned px_blocks = (unsigned)((flow + kBlock - 1) / kBlock);
  if (scheme == EBOS_FLOW_SAME) {
    hipLaunchKernelGGL(broadcast_kernel<T>, dim3(px_blocks, B), dim3(kBlock), 0, st, in, flow, n_bins, voxel, has_clamp, (T)clamp, out);
    EBOS_CHECK_LAUNCH(who);
    return EBOS_OK;
  }
  // the torch Burgers constructor steps once more below bin 0 and stores that in bin -1 = the last one; the forward chain overwrites
  // it unless t0 is the last bin, so only then is the step taken
  const bool wrap = wrap_last && t0 == n_bins - 1;
  const int k_back = t0 + (wrap ? 1 : 0), k_forw = n_bins - 1 - t0;
  const bool fits = k_back <= kHaloCap && k_forw <= kHaloCap;
  EBOS_REQUIRE(route != EBOS_FLOW_ROUTE_FUSED || fits, "%s: %d and %d steps do not fit a halo of %d", who, k_back, k_forw, kHaloCap);
  const double dt = 1.0 / (double)n_bins;
  const Step<T> s = make_step<T>(scheme, H, W, dt, 1.0, 1.0);
  if (route == EBOS_FLOW_ROUTE_FUSED || (route == EBOS_FLOW_ROUTE_AUTO && fits)) {
    Chain c;
    c.B = B; c.T = n_bins; c.t0 = t0; c.k_back = k_back; c.k_forw = k_forw;
    c.wrap_bin = wrap ? n_bins - 1 : -1;
    c.write_t0 = !wrap;
    c.has_clamp = has_clamp;
    hipLaunchKernelGGL(chain_kernel<T>, dim3((W + kTile - 1) / kTile, (H + kTile - 1) / kTile, 2 * B), dim3(kBlock), 0, st, s, c, (T)clamp, in, out);
    EBOS_CHECK_LAUNCH(who);
    return EBOS_OK;
  }
  // the first step of either direction reads the input, the later ones the bin before them; no step runs in place
  const dim3 grid((unsigned)((plane + kBlock - 1) / kBlock), B);
  if (!wrap) {
    hipLaunchKernelGGL(broadcast_kernel<T>, dim3(px_blocks, B), dim3(kBlock), 0, st, in, flow, 1, voxel, 0, T(0), out + (int64_t)t0 * flow);
    EBOS_CHECK_LAUNCH(who);
  }
  for (int step = 1; step <= k_back; ++step) {
    const int to = t0 - step < 0 ? n_bins - 1 : t0 - step;   // (the wrapped step reads bin 0 and writes bin t0 = the last one)
    const T* from = step == 1 ? in : out + (int64_t)(t0 - step + 1) * flow;
    hipLaunchKernelGGL(step_kernel<T>, grid, dim3(kBlock), 0, st, s, T(-1), from, step == 1 ? flow : voxel, out + (int64_t)to * flow, voxel);
    EBOS_CHECK_LAUNCH(who);
  }
  for (int step = 1; step <= k_forw; ++step) {
    const T* from = step == 1 ? in : out + (int64_t)(t0 + step - 1) * flow;
    hipLaunchKernelGGL(step_kernel<T>, grid, dim3(kBlock), 0, st, s, T(1), from, step == 1 ? flow : voxel, out + (int64_t)(t0 + step) * flow, voxel);
    EBOS_CHECK_LAUNCH(who);
  }
  if (has_clamp) {
    hipLaunchKernelGGL(clamp_kernel<T>, dim3(stream_grid((int64_t)B * voxel, kBlock)), dim3(kBlock), 0, st, out, (int64_t)B * voxel, (T)clamp);
    EBOS_CHECK_LAUNCH(who);
  }
  return EBOS_OK;
}

template <typename T>
int bilinear(const char* who, int B, int n_bins, int H, int W, const T* in, T* out, int t_off, int denom, double dt_single, int has_clamp,
             double clamp, ebos_stream_t stream) {
  if (int rc = check_step<T>(who, B, H, W, in, out, dt_single, 1.0, 1.0)) return rc;
  EBOS_REQUIRE(n_bins > 0 && (int64_t)B * n_bins <= 65535, "%s: %d flows x %d bins (at most 65535 bins in all)", who, B, n_bins);
  EBOS_REQUIRE(denom >= 0, "%s: denominator %d", who, denom);
  EBOS_REQUIRE(!has_clamp || clamp == clamp, "%s: the clamp must be a number", who);
  const hipStream_t st = as_stream(stream);
  const int64_t plane = (int64_t)H * W, total = (int64_t)B * n_bins * 2 * plane;
  EBOS_REQUIRE(disjoint(in, (int64_t)B * 2 * plane, static_cast<const T*>(out), total), "%s: out overlaps the flows", who);
  if (hipMemsetAsync(out, 0, sizeof(T) * (size_t)total, st) != hipSuccess) {
    set_error("%s: hipMemsetAsync failed", who);
    return EBOS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(bilinear_kernel<T>, dim3((unsigned)((plane + kBlock - 1) / kBlock), B * n_bins), dim3(kBlock), 0, st, in, H, W, n_bins, t_off,
                     denom, dt_single, out);
  EBOS_CHECK_LAUNCH(who);
  if (has_clamp) {
    hipLaunchKernelGGL(clamp_kernel<T>, dim3(stream_grid(total, kBlock)), dim3(kBlock), 0, st, out, total, (T)clamp);
    EBOS_CHECK_LAUNCH(who);
  }
  return EBOS_OK;
}

template <typename T>
int truncate_mean(const char* who, int n_bins, int H, int W, const T* voxel, double* out, ebos_stream_t stream) {
  EBOS_REQUIRE(n_bins > 0 && H > 0 && W > 0 && (int64_t)H * W <= 2147483647ll, "%s: bad voxel %d x 2 x %d x %d", who, n_bins, H, W);
  EBOS_REQUIRE(voxel && out, "%s: NULL buffer", who);
  const int64_t plane = (int64_t)H * W;
  hipLaunchKernelGGL(truncate_kernel<T>, dim3((unsigned)((plane + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), voxel, n_bins, plane, out);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

using namespace ebos;

extern "C" {

int ebos_flow_voxel_halo_cap(void) { return kHaloCap; }

int ebos_flow_voxel_advect_f32(int scheme, int B, int T, int H, int W, const float* flow, float* out, int t0_index, int has_clamp,
                               double clamp, int wrap_last, int route, ebos_stream_t stream) {
  return advect<float>("ebos_flow_voxel_advect_f32", scheme, B, T, H, W, flow, out, t0_index, has_clamp, clamp, wrap_last, route, stream);
}
int ebos_flow_voxel_advect_f64(int scheme, int B, int T, int H, int W, const double* flow, double* out, int t0_index, int has_clamp,
                               double clamp, int wrap_last, int route, ebos_stream_t stream) {
  return advect<double>("ebos_flow_voxel_advect_f64", scheme, B, T, H, W, flow, out, t0_index, has_clamp, clamp, wrap_last, route, stream);
}

int ebos_flow_upwind_step_f32(int B, int H, int W, const float* flow, float* out, double dt, double dx, double dy, ebos_stream_t stream) {
  return single_step<float>("ebos_flow_upwind_step_f32", EBOS_FLOW_UPWIND, B, H, W, flow, out, dt, dx, dy, stream);
}
int ebos_flow_upwind_step_f64(int B, int H, int W, const double* flow, double* out, double dt, double dx, double dy, ebos_stream_t stream) {
  return single_step<double>("ebos_flow_upwind_step_f64", EBOS_FLOW_UPWIND, B, H, W, flow, out, dt, dx, dy, stream);
}
int ebos_flow_burgers_step_f32(int B, int H, int W, const float* flow, float* out, double dt, double dx, double dy, ebos_stream_t stream) {
  return single_step<float>("ebos_flow_burgers_step_f32", EBOS_FLOW_BURGERS, B, H, W, flow, out, dt, dx, dy, stream);
}
int ebos_flow_burgers_step_f64(int B, int H, int W, const double* flow, double* out, double dt, double dx, double dy, ebos_stream_t stream) {
  return single_step<double>("ebos_flow_burgers_step_f64", EBOS_FLOW_BURGERS, B, H, W, flow, out, dt, dx, dy, stream);
}

int ebos_flow_voxel_propagate_bilinear_f32(int B, int T, int H, int W, const float* flow, float* out, int t_offset, int denominator,
                                           double dt, int has_clamp, double clamp, ebos_stream_t stream) {
  return bilinear<float>("ebos_flow_voxel_propagate_bilinear_f32", B, T, H, W, flow, out, t_offset, denominator, dt, has_clamp, clamp, stream);
}
int ebos_flow_voxel_propagate_bilinear_f64(int B, int T, int H, int W, const double* flow, double* out, int t_offset, int denominator,
                                           double dt, int has_clamp, double clamp, ebos_stream_t stream) {
  return bilinear<double>("ebos_flow_voxel_propagate_bilinear_f64", B, T, H, W, flow, out, t_offset, denominator, dt, has_clamp, clamp, stream);
}

int ebos_flow_voxel_truncate_mean_f32(int T, int H, int W, const float* voxel, double* out, ebos_stream_t stream) {
  return truncate_mean<float>("ebos_flow_voxel_truncate_mean_f32", T, H, W, voxel, out, stream);
}
int ebos_flow_voxel_truncate_mean_f64(int T, int H, int W, const double* voxel, double* out, ebos_stream_t stream) {
  return truncate_mean<double>("ebos_flow_voxel_truncate_mean_f64", T, H, W, voxel, out, stream);
}

}  // extern "C"
