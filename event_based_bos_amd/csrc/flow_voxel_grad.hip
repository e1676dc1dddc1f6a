// flow_voxel_grad.hip -- the backward of flow_voxel.hip with respect to the flow at t0: adjoints of one upwind / Burgers step, of the
// whole chain of steps of a voxel, of the "same" copy and of the bilinear propagation, float32 and float64, batched.
//
// Every kernel gathers: an input pixel sums what its own outputs and those of its neighbours (or, for the bilinear vote, its four
// cells) hand back, in a fixed order, without atomics -- two runs give the same bits.  The derivative rules are torch's
// (flow_voxel_adjoint.h): half the gradient on each side of a tie of maximum / minimum, none through sign() and floor().
//
// The chain:  W_0 = flow,  W_s = step(W_{s-1}, -+1/T) = bin t0 -+ s of the UNCLAMPED voxel;  the clamp comes last, so bin W_s hands
// its upstream gradient on where -c <= W_s <= c.  Walking from the outer bin towards t0,
//     G_k = up_k,   G_s = up_s + J(W_s)^T G_{s+1},   d flow = up_0 + J(W_0)^T G_1 [above t0] + J(W_0)^T G_1 [below t0].
// The fused route keeps the running gradient G and the bin W_s of a tile with its halo side by side in LDS and runs the k steps of a
// direction there -- G_s on the tile grown by s pixels, which reads G_{s+1} and W_s on the tile grown by s + 1 -- both directions one
// after the other in one workgroup, which owns its tile of the result.  The tile is 32 x 32 in float32 (36 KB of LDS, 4 workgroups
// per CU) and 24 x 24 in float64 (50 KB, 3 per CU): four planes of the float64 48 x 48 region would be 72 KB, beyond the 64 KB a
// workgroup gets without asking for more.  Longer chains take one launch per step through two scratch fields.
#include <math.h>

#include "common.h"

#define EBOS_HD __device__ __forceinline__
#include "flow_voxel_adjoint.h"

#pragma clang fp contract(off)   // the bilinear adjoint recomputes the forward's cells: the same roundings, the same floor()

namespace ebos {
namespace {

using namespace flow_adjoint;

constexpr int kBlock = 256;
constexpr int kHaloCap = EBOS_FLOW_VOXEL_HALO_CAP;

template <typename T>
struct AdjointTile {
  static constexpr int kTile = sizeof(T) == 4 ? 32 : 24;
  static constexpr int kRegion = kTile + 2 * kHaloCap;                           // the tile with its largest halo
  static constexpr int kGrown = kTile + 2 * (kHaloCap - 1);                      // the widest square a step updates
  static constexpr int kCells = (kGrown * kGrown + kBlock - 1) / kBlock;         // cells per lane at most: 9 (float), 6 (double)
  static_assert(sizeof(T) * 4 * kRegion * kRegion <= 64 * 1024, "bin and gradient of the tile with its halo have to fit the workgroup's LDS");
};

// a field [.., 2, H, W] with a batch stride of its own: a flow, a bin of a voxel, a scratch field
template <typename T>
struct Field {
  const T* p;
  int64_t bs;
};

// ---------------------------------------------------------------------------------------------------- one launch per step
// out[b] = (add ? add[b] * pass(add_mask[b]) : 0) + J(sign * w[b])^T (g[b] * pass(g_mask[b]));  a mask field with p == NULL passes all
template <typename T>
__global__ __launch_bounds__(kBlock) void step_adjoint_kernel(StepGeometry<T> s, T sign, Field<T> w, Field<T> g, Field<T> g_mask, Field<T> add,
                                                              Field<T> add_mask, T clamp, T* out, int64_t out_bs) {
  const int64_t plane = (int64_t)s.H * s.W;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= plane) return;
  const int i = (int)(p / s.W), j = (int)(p % s.W);
  const int b = blockIdx.y;
  const T* wp = w.p + b * w.bs;
  const T* gp = g.p + b * g.bs;
  const T* gm = g_mask.p ? g_mask.p + b * g_mask.bs : nullptr;
  auto F = [&](int c, int ii, int jj) { return wp[c * plane + (int64_t)ii * s.W + jj] * sign; };
  auto G = [&](int c, int ii, int jj) {
    const int64_t n = c * plane + (int64_t)ii * s.W + jj;
    return gm ? gp[n] * clamp_pass(gm[n], 1, clamp) : gp[n];
  };
  T du, dv;
  step_adjoint_pixel(s, F, G, i, j, &du, &dv);
  if (add.p) {
    const T* ap = add.p + b * add.bs;
    T au = ap[p], av = ap[plane + p];
    if (add_mask.p) {
      const T* am = add_mask.p + b * add_mask.bs;
      au *= clamp_pass(am[p], 1, clamp);
      av *= clamp_pass(am[plane + p], 1, clamp);
    }
    du = au + du;
    dv = av + dv;
  }
  T* dst = out + b * out_bs;
  dst[p] = du;
  dst[plane + p] = dv;
}

// out[b] = sum_t grad[b, t] * pass(in[b]), the bins in index order: scheme "same", and a chain without any step (n_bins = 1)
template <typename T>
__global__ __launch_bounds__(kBlock) void same_adjoint_kernel(const T* __restrict__ in, const T* __restrict__ grad, int64_t n, int n_bins, int64_t grad_bs,
                                                              int has_clamp, T clamp, T* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const T* g = grad + (int64_t)blockIdx.y * grad_bs + p;
  T sum = g[0];
  for (int t = 1; t < n_bins; ++t) sum += g[(int64_t)t * n];
  out[(int64_t)blockIdx.y * n + p] = sum * clamp_pass(in[(int64_t)blockIdx.y * n + p], has_clamp, clamp);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void clamp_copy_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t n, T c) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
    T x = in[p];
    if (x == x) {   // np.clip / torch.clamp: min(max(x, -c), c), NaN comes through
      const T lo = -c;
      x = x > lo ? x : lo;
      x = x < c ? x : c;
    }
    out[p] = x;
  }
}

// ---------------------------------------------------------------------------------------------------- the chain in LDS
struct ChainAdjoint {
  int T, t0;
  int k_back, k_forw;   // steps below and above t0, each <= kHaloCap
  int wrap;             // the torch Burgers constructor's extra step: bin -1 is bin T - 1, and the flow itself is no bin
  int has_clamp;
};

// grid (tiles along W, tiles along H, B)
template <typename T>
__global__ __launch_bounds__(kBlock) void chain_adjoint_kernel(StepGeometry<T> s, ChainAdjoint c, T clamp, const T* __restrict__ in,
                                                               const T* __restrict__ voxel, const T* __restrict__ grad, T* out) {
  constexpr int kTile = AdjointTile<T>::kTile, kRegion = AdjointTile<T>::kRegion, kCells = AdjointTile<T>::kCells;
  __shared__ T wt[2][kRegion][kRegion];   // W_s, sign-swapped
  __shared__ T gt[2][kRegion][kRegion];   // G_{s+1}
  const int b = blockIdx.z;
  const int H = s.H, W = s.W;
  const int64_t plane = (int64_t)H * W, flow = 2 * plane;
  const T* src = in + (int64_t)b * flow;
  const T* vox = voxel + (int64_t)b * c.T * flow;
  const T* gup = grad + (int64_t)b * c.T * flow;
  T* dst = out + (int64_t)b * flow;
  bool first = true;   // nothing stored in dst yet

  for (int dir = 0; dir < 2; ++dir) {
    const int k = dir ? c.k_back : c.k_forw;
    if (k == 0) continue;
    const T sign = dir ? T(-1) : T(1);
    const int i0 = blockIdx.y * kTile - k, j0 = blockIdx.x * kTile - k;   // image position of wt[.][0][0]
    const int R = kTile + 2 * k;
    auto bin_of = [&](int step) {
      const int bin = dir ? c.t0 - step : c.t0 + step;
      return bin < 0 ? c.T - 1 : bin;
    };
    {   // G_k = up_k on the tile grown by k
      const int64_t at = (int64_t)bin_of(k) * flow;
      for (int n = threadIdx.x; n < R * R; n += kBlock) {
        const int ri = n / R, rj = n % R, i = i0 + ri, j = j0 + rj;
        if (i < 0 || i >= H || j < 0 || j >= W) continue;               // (never read: a pixel asks for pixels of the image only)
        const int64_t px = at + (int64_t)i * W + j;
        gt[0][ri][rj] = gup[px] * clamp_pass(vox[px], c.has_clamp, clamp);
        gt[1][ri][rj] = gup[px + plane] * clamp_pass(vox[px + plane], c.has_clamp, clamp);
      }
    }
    auto F = [&](int comp, int i, int j) { return wt[comp][i - i0][j - j0]; };
    auto G = [&](int comp, int i, int j) { return gt[comp][i - i0][j - j0]; };
    for (int step = k - 1; step >= 0; --step) {
      {   // W_step on the tile grown by step + 1
        const T* from = step == 0 ? src : vox + (int64_t)bin_of(step) * flow;
        const int wl = kTile + 2 * (step + 1), off = k - step - 1;
        for (int n = threadIdx.x; n < wl * wl; n += kBlock) {
          const int ri = off + n / wl, rj = off + n % wl, i = i0 + ri, j = j0 + rj;
          if (i < 0 || i >= H || j < 0 || j >= W) continue;
          const int64_t px = (int64_t)i * W + j;
          wt[0][ri][rj] = from[px] * sign;
          wt[1][ri][rj] = from[px + plane] * sign;
        }
      }
      __syncthreads();
      const int wa = kTile + 2 * step, off = k - step;                   // the tile grown by step pixels
      const int64_t at = (int64_t)bin_of(step) * flow;
      T nu[kCells], nv[kCells];
#pragma unroll
      for (int q = 0; q < kCells; ++q) {
        const int n = threadIdx.x + q * kBlock;
        if (n >= wa * wa) continue;
        const int ri = off + n / wa, rj = off + n % wa, i = i0 + ri, j = j0 + rj;
        if (i < 0 || i >= H || j < 0 || j >= W) continue;
        step_adjoint_pixel(s, F, G, i, j, &nu[q], &nv[q]);
        const int64_t px = (int64_t)i * W + j;
        if (step > 0) {   // + up_step; the bin is W_step itself, and the clamp's bounds are symmetric: the sign swap does not matter
          nu[q] = gup[at + px] * clamp_pass(wt[0][ri][rj], c.has_clamp, clamp) + nu[q];
          nv[q] = gup[at + px + plane] * clamp_pass(wt[1][ri][rj], c.has_clamp, clamp) + nv[q];
        } else {          // the tile itself: the result, on top of up_0 or of what the other direction left
          T bu = T(0), bv = T(0);
          if (!first) {
            bu = dst[px];
            bv = dst[px + plane];
          } else if (!c.wrap) {
            bu = gup[at + px] * clamp_pass(wt[0][ri][rj], c.has_clamp, clamp);
            bv = gup[at + px + plane] * clamp_pass(wt[1][ri][rj], c.has_clamp, clamp);
          }
          dst[px] = bu + nu[q];
          dst[px + plane] = bv + nv[q];
        }
      }
      __syncthreads();
      if (step == 0) break;
#pragma unroll
      for (int q = 0; q < kCells; ++q) {
        const int n = threadIdx.x + q * kBlock;
        if (n >= wa * wa) continue;
        const int ri = off + n / wa, rj = off + n % wa, i = i0 + ri, j = j0 + rj;
        if (i < 0 || i >= H || j < 0 || j >= W) continue;
        gt[0][ri][rj] = nu[q];
        gt[1][ri][rj] = nv[q];
      }
    }
    first = false;
  }
}

// ---------------------------------------------------------------------------------------------------- bilinear propagation
// grid (pixels, B).  Source pixel (i, j) voted w_q f_c into its four cells in every bin (bilinear_kernel of flow_voxel.hip: the same
// expressions, so the same cells).  Its gradient is, summed over the bins in index order,
//     d f_0 = sum_q w_q g_0[cell_q] + dt sum_q (d w_q / d fx) (f_0 g_0[cell_q] + f_1 g_1[cell_q]),   d f_1 likewise with fy,
// with the reference's pairing of weights and cells and its inside masks; floor() has no gradient.  g is the upstream gradient through
// the clamp of the finished (unclamped) cell.
template <typename T>
__global__ __launch_bounds__(kBlock) void bilinear_adjoint_kernel(const T* __restrict__ in, const T* __restrict__ voxel, const T* __restrict__ grad, int H, int W,
                                                                  int n_bins, int t_off, int denom, double dt_single, int has_clamp, T clamp,
                                                                  T* __restrict__ out) {
  const int64_t plane = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.y;
  const int i = (int)(p / W), j = (int)(p % W);
  const T* src = in + (int64_t)b * 2 * plane;
  const T f0 = src[p], f1 = src[plane + p];
  T acc0 = T(0), acc1 = T(0);
  for (int t = 0; t < n_bins; ++t) {
    const T dt = (T)(denom > 0 ? (double)(t - t_off) / (double)denom : dt_single);
    const int64_t bin = ((int64_t)b * n_bins + t) * 2 * plane;
    const T x = f0 * dt + (T)i, y = f1 * dt + (T)j;
    const T x1 = floor(x + (T)1e-8), y1 = floor(y + (T)1e-8);
    const T fx = x - x1, fy = y - y1;
    const T w[4] = {(T(1) - fx) * (T(1) - fy), (T(1) - fx) * fy, fx * (T(1) - fy), fx * fy};
    const T wx[4] = {-(T(1) - fy), -fy, T(1) - fy, fy};   // d w / d fx
    const T wy[4] = {-(T(1) - fx), T(1) - fx, -fx, fx};   // d w / d fy
    const T cx[4] = {x1, x1 + T(1), x1, x1 + T(1)}, cy[4] = {y1, y1, y1 + T(1), y1 + T(1)};
    T direct0 = T(0), direct1 = T(0), via_x = T(0), via_y = T(0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool inside = T(0) <= cy[q] && cy[q] < (T)W && T(0) <= cx[q] && cx[q] < (T)H;
      if (!inside) continue;
      const int64_t cell = bin + (int64_t)cx[q] * W + (int64_t)cy[q];
      T g0 = grad[cell], g1 = grad[cell + plane];
      if (has_clamp) {
        g0 *= clamp_pass(voxel[cell], 1, clamp);
        g1 *= clamp_pass(voxel[cell + plane], 1, clamp);
      }
      direct0 += w[q] * g0;
      direct1 += w[q] * g1;
      const T e = f0 * g0 + f1 * g1;
      via_x += wx[q] * e;
      via_y += wy[q] * e;
    }
    acc0 += direct0 + dt * via_x;
    acc1 += direct1 + dt * via_y;
  }
  T* dst = out + (int64_t)b * 2 * plane;
  dst[p] = acc0;
  dst[plane + p] = acc1;
}

// ---------------------------------------------------------------------------------------------------- hosts
template <typename T>
int check_fields(const char* who, int B, int H, int W) {
  EBOS_REQUIRE(B > 0 && B <= 32767 && H > 0 && W > 0, "%s: %d flows of %d x %d (1 .. 32767 flows)", who, B, H, W);
  EBOS_REQUIRE((int64_t)H * W <= 2147483647ll, "%s: %d x %d pixels", who, H, W);
  return EBOS_OK;
}

template <typename T>
bool disjoint(const T* a, int64_t na, const T* b, int64_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 + sizeof(T) * (uint64_t)na <= b0 || b0 + sizeof(T) * (uint64_t)nb <= a0;
}

template <typename T>
StepGeometry<T> make_geometry(int scheme, int H, int W, double dt, double dx, double dy) {
  StepGeometry<T> s;
  s.scheme = scheme; s.H = H; s.W = W;
  s.dt = (T)fabs(dt); s.dx = (T)dx; s.dy = (T)dy;
  return s;
}

template <typename T>
int step_adjoint(const char* who, int scheme, int B, int H, int W, const T* flow, const T* grad_out, T* grad_in, double dt, double dx, double dy,
                 ebos_stream_t stream) {
  if (int rc = check_fields<T>(who, B, H, W)) return rc;
  EBOS_REQUIRE(scheme == EBOS_FLOW_UPWIND || scheme == EBOS_FLOW_BURGERS, "%s: unknown scheme %d", who, scheme);
  EBOS_REQUIRE(flow && grad_out && grad_in, "%s: NULL buffer", who);
  EBOS_REQUIRE(dt == dt && dx == dx && dy == dy && dt != 0.0, "%s: dt, dx and dy must be numbers and dt not 0 (the identity)", who);
  const int64_t plane = (int64_t)H * W, total = (int64_t)B * 2 * plane;
  EBOS_REQUIRE(disjoint(flow, total, static_cast<const T*>(grad_in), total) && disjoint(grad_out, total, static_cast<const T*>(grad_in), total),
               "%s: grad_in overlaps an input; a pixel reads its neighbours", who);
  const Field<T> none{nullptr, 0};
  hipLaunchKernelGGL(step_adjoint_kernel<T>, dim3((unsigned)((plane + kBlock - 1) / kBlock), B), dim3(kBlock), 0, as_stream(stream),
                     make_geometry<T>(scheme, H, W, dt, dx, dy), dt < 0.0 ? T(-1) : T(1), Field<T>{flow, 2 * plane}, Field<T>{grad_out, 2 * plane}, none,
                     none, none, T(0), grad_in, 2 * plane);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

struct Plan {
  int k_back, k_forw;
  bool wrap, fused;
};

int plan_of(const char* who, int scheme, int n_bins, int t0, int wrap_last, int route, Plan* plan) {
  EBOS_REQUIRE(scheme == EBOS_FLOW_UPWIND || scheme == EBOS_FLOW_BURGERS || scheme == EBOS_FLOW_SAME, "%s: unknown scheme %d", who, scheme);
  EBOS_REQUIRE(n_bins > 0 && t0 >= 0 && t0 < n_bins, "%s: bin %d of %d", who, t0, n_bins);
  EBOS_REQUIRE(route >= EBOS_FLOW_ROUTE_AUTO && route <= EBOS_FLOW_ROUTE_STEPS, "%s: unknown route %d", who, route);
  plan->wrap = wrap_last && scheme == EBOS_FLOW_BURGERS && t0 == n_bins - 1;   // as the forward: only where no forward step overwrites it
  plan->k_back = scheme == EBOS_FLOW_SAME ? 0 : t0 + (plan->wrap ? 1 : 0);
  plan->k_forw = scheme == EBOS_FLOW_SAME ? 0 : n_bins - 1 - t0;
  const bool fits = plan->k_back <= kHaloCap && plan->k_forw <= kHaloCap;
  EBOS_REQUIRE(route != EBOS_FLOW_ROUTE_FUSED || fits, "%s: %d and %d steps do not fit a halo of %d", who, plan->k_back, plan->k_forw, kHaloCap);
  plan->fused = route == EBOS_FLOW_ROUTE_FUSED || (route == EBOS_FLOW_ROUTE_AUTO && fits);
  return EBOS_OK;
}

template <typename T>
int advect_adjoint(const char* who, int scheme, int B, int n_bins, int H, int W, const T* in, const T* voxel, const T* grad, T* out, int t0,
                   int has_clamp, double clamp, int wrap_last, int route, T* workspace, ebos_stream_t stream) {
  if (int rc = check_fields<T>(who, B, H, W)) return rc;
  Plan plan;
  if (int rc = plan_of(who, scheme, n_bins, t0, wrap_last, route, &plan)) return rc;
  EBOS_REQUIRE(in && grad && out && (voxel || scheme == EBOS_FLOW_SAME), "%s: NULL buffer", who);
  EBOS_REQUIRE(!has_clamp || clamp == clamp, "%s: the clamp must be a number", who);
  const hipStream_t st = as_stream(stream);
  const int64_t plane = (int64_t)H * W, flow = 2 * plane, vol = (int64_t)n_bins * flow;
  EBOS_REQUIRE(disjoint(in, (int64_t)B * flow, static_cast<const T*>(out), (int64_t)B * flow) &&
                   disjoint(grad, (int64_t)B * vol, static_cast<const T*>(out), (int64_t)B * flow) &&
                   (!voxel || disjoint(voxel, (int64_t)B * vol, static_cast<const T*>(out), (int64_t)B * flow)),
               "%s: out overlaps an input", who);
  const unsigned px_blocks = (unsigned)((flow + kBlock - 1) / kBlock);
  if (plan.k_back == 0 && plan.k_forw == 0) {   // "same": every bin is the flow; a voxel of one bin: bin t0 is
    const bool same = scheme == EBOS_FLOW_SAME;
    hipLaunchKernelGGL(same_adjoint_kernel<T>, dim3(px_blocks, B), dim3(kBlock), 0, st, in, same ? grad : grad + (int64_t)t0 * flow, flow,
                       same ? n_bins : 1, vol, has_clamp, (T)clamp, out);
    EBOS_CHECK_LAUNCH(who);
    return EBOS_OK;
  }
  const StepGeometry<T> s = make_geometry<T>(scheme, H, W, 1.0 / (double)n_bins, 1.0, 1.0);
  if (plan.fused) {
    constexpr int kTile = AdjointTile<T>::kTile;
    ChainAdjoint c;
    c.T = n_bins; c.t0 = t0; c.k_back = plan.k_back; c.k_forw = plan.k_forw; c.wrap = plan.wrap; c.has_clamp = has_clamp;
    EBOS_REQUIRE((H + kTile - 1) / kTile <= 65535, "%s: %d rows are more than 65535 tiles", who, H);
    hipLaunchKernelGGL(chain_adjoint_kernel<T>, dim3((W + kTile - 1) / kTile, (H + kTile - 1) / kTile, B), dim3(kBlock), 0, st, s, c, (T)clamp, in,
                       voxel, grad, out);
    EBOS_CHECK_LAUNCH(who);
    return EBOS_OK;
  }
  EBOS_REQUIRE(workspace, "%s: the per-step route needs its workspace", who);
  EBOS_REQUIRE(disjoint(static_cast<const T*>(workspace), 2 * (int64_t)B * flow, static_cast<const T*>(out), (int64_t)B * flow),
               "%s: the workspace overlaps out", who);
  T* const ws[2] = {workspace, workspace + (int64_t)B * flow};
  const Field<T> none{nullptr, 0};
  const dim3 grid((unsigned)((plane + kBlock - 1) / kBlock), B);
  bool first = true;
  for (int dir = 0; dir < 2; ++dir) {
    const int k = dir ? plan.k_back : plan.k_forw;
    if (k == 0) continue;
    auto bin_of = [&](int step) {
      const int bin = dir ? t0 - step : t0 + step;
      return bin < 0 ? n_bins - 1 : bin;
    };
    const auto bin_field = [&](const T* base, int step) { return Field<T>{base + (int64_t)bin_of(step) * flow, vol}; };
    Field<T> g = bin_field(grad, k), g_mask = has_clamp ? bin_field(voxel, k) : none;
    for (int step = k - 1; step >= 0; --step) {
      Field<T> w, add, add_mask = none;
      T* to;
      if (step > 0) {
        w = bin_field(voxel, step);
        add = bin_field(grad, step);
        if (has_clamp) add_mask = w;
        to = ws[step & 1];
      } else {
        w = Field<T>{in, flow};
        if (!first) {
          add = Field<T>{out, flow};
        } else if (plan.wrap) {
          add = none;
        } else {
          add = bin_field(grad, 0);
          if (has_clamp) add_mask = w;
        }
        to = out;
      }
      hipLaunchKernelGGL(step_adjoint_kernel<T>, grid, dim3(kBlock), 0, st, s, dir ? T(-1) : T(1), w, g, g_mask, add, add_mask, (T)clamp, to, flow);
      EBOS_CHECK_LAUNCH(who);
      g = Field<T>{to, flow};
      g_mask = none;
    }
    first = false;
  }
  return EBOS_OK;
}

template <typename T>
int bilinear_adjoint(const char* who, int B, int n_bins, int H, int W, const T* in, const T* voxel, const T* grad, T* out, int t_off, int denom,
                     double dt_single, int has_clamp, double clamp, ebos_stream_t stream) {
  if (int rc = check_fields<T>(who, B, H, W)) return rc;
  EBOS_REQUIRE(n_bins > 0 && (int64_t)B * n_bins <= 65535, "%s: %d flows x %d bins (at most 65535 bins in all)", who, B, n_bins);
  EBOS_REQUIRE(denom >= 0 && dt_single == dt_single, "%s: denominator %d, dt %g", who, denom, dt_single);
  EBOS_REQUIRE(in && grad && out && (voxel || !has_clamp), "%s: NULL buffer", who);
  EBOS_REQUIRE(!has_clamp || clamp == clamp, "%s: the clamp must be a number", who);
  const int64_t plane = (int64_t)H * W, flow = 2 * plane, vol = (int64_t)n_bins * flow;
  EBOS_REQUIRE(disjoint(in, (int64_t)B * flow, static_cast<const T*>(out), (int64_t)B * flow) &&
                   disjoint(grad, (int64_t)B * vol, static_cast<const T*>(out), (int64_t)B * flow) &&
                   (!voxel || disjoint(voxel, (int64_t)B * vol, static_cast<const T*>(out), (int64_t)B * flow)),
               "%s: out overlaps an input", who);
  hipLaunchKernelGGL(bilinear_adjoint_kernel<T>, dim3((unsigned)((plane + kBlock - 1) / kBlock), B), dim3(kBlock), 0, as_stream(stream), in, voxel, grad,
                     H, W, n_bins, t_off, denom, dt_single, has_clamp, (T)clamp, out);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

template <typename T>
int clamp_copy(const char* who, int64_t n, const T* in, T* out, double clamp, ebos_stream_t stream) {
  EBOS_REQUIRE(n > 0 && in && out, "%s: %lld values", who, (long long)n);
  EBOS_REQUIRE(clamp == clamp, "%s: the clamp must be a number", who);
  EBOS_REQUIRE(disjoint(in, n, static_cast<const T*>(out), n), "%s: out overlaps the input", who);
  hipLaunchKernelGGL(clamp_copy_kernel<T>, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, as_stream(stream), in, out, n, (T)clamp);
  EBOS_CHECK_LAUNCH(who);
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

using namespace ebos;

extern "C" {

int64_t ebos_flow_voxel_advect_adjoint_workspace(int scheme, int B, int T, int H, int W, int t0_index, int wrap_last, int route) {
  Plan plan;
  if (B <= 0 || H <= 0 || W <= 0 || plan_of("ebos_flow_voxel_advect_adjoint_workspace", scheme, T, t0_index, wrap_last, route, &plan)) return -1;
  return plan.fused || (plan.k_back == 0 && plan.k_forw == 0) ? 0 : 4 * (int64_t)B * H * W;
}

int ebos_flow_upwind_step_adjoint_f32(int B, int H, int W, const float* flow, const float* grad_out, float* grad_in, double dt, double dx, double dy,
                                      ebos_stream_t stream) {
  return step_adjoint<float>("ebos_flow_upwind_step_adjoint_f32", EBOS_FLOW_UPWIND, B, H, W, flow, grad_out, grad_in, dt, dx, dy, stream);
}
int ebos_flow_upwind_step_adjoint_f64(int B, int H, int W, const double* flow, const double* grad_out, double* grad_in, double dt, double dx, double dy,
                                      ebos_stream_t stream) {
  return step_adjoint<double>("ebos_flow_upwind_step_adjoint_f64", EBOS_FLOW_UPWIND, B, H, W, flow, grad_out, grad_in, dt, dx, dy, stream);
}
int ebos_flow_burgers_step_adjoint_f32(int B, int H, int W, const float* flow, const float* grad_out, float* grad_in, double dt, double dx, double dy,
                                       ebos_stream_t stream) {
  return step_adjoint<float>("ebos_flow_burgers_step_adjoint_f32", EBOS_FLOW_BURGERS, B, H, W, flow, grad_out, grad_in, dt, dx, dy, stream);
}
int ebos_flow_burgers_step_adjoint_f64(int B, int H, int W, const double* flow, const double* grad_out, double* grad_in, double dt, double dx, double dy,
                                       ebos_stream_t stream) {
  return step_adjoint<double>("ebos_flow_burgers_step_adjoint_f64", EBOS_FLOW_BURGERS, B, H, W, flow, grad_out, grad_in, dt, dx, dy, stream);
}

int ebos_flow_voxel_advect_adjoint_f32(int scheme, int B, int T, int H, int W, const float* flow, const float* voxel, const float* grad_voxel,
                                       float* grad_flow, int t0_index, int has_clamp, double clamp, int wrap_last, int route, float* workspace,
                                       ebos_stream_t stream) {
  return advect_adjoint<float>("ebos_flow_voxel_advect_adjoint_f32", scheme, B, T, H, W, flow, voxel, grad_voxel, grad_flow, t0_index, has_clamp, clamp,
                               wrap_last, route, workspace, stream);
}
int ebos_flow_voxel_advect_adjoint_f64(int scheme, int B, int T, int H, int W, const double* flow, const double* voxel, const double* grad_voxel,
                                       double* grad_flow, int t0_index, int has_clamp, double clamp, int wrap_last, int route, double* workspace,
                                       ebos_stream_t stream) {
  return advect_adjoint<double>("ebos_flow_voxel_advect_adjoint_f64", scheme, B, T, H, W, flow, voxel, grad_voxel, grad_flow, t0_index, has_clamp, clamp,
                                wrap_last, route, workspace, stream);
}

int ebos_flow_voxel_propagate_bilinear_adjoint_f32(int B, int T, int H, int W, const float* flow, const float* voxel, const float* grad_voxel,
                                                   float* grad_flow, int t_offset, int denominator, double dt, int has_clamp, double clamp,
                                                   ebos_stream_t stream) {
  return bilinear_adjoint<float>("ebos_flow_voxel_propagate_bilinear_adjoint_f32", B, T, H, W, flow, voxel, grad_voxel, grad_flow, t_offset, denominator,
                                 dt, has_clamp, clamp, stream);
}
int ebos_flow_voxel_propagate_bilinear_adjoint_f64(int B, int T, int H, int W, const double* flow, const double* voxel, const double* grad_voxel,
                                                   double* grad_flow, int t_offset, int denominator, double dt, int has_clamp, double clamp,
                                                   ebos_stream_t stream) {
  return bilinear_adjoint<double>("ebos_flow_voxel_propagate_bilinear_adjoint_f64", B, T, H, W, flow, voxel, grad_voxel, grad_flow, t_offset, denominator,
                                  dt, has_clamp, clamp, stream);
}

int ebos_flow_voxel_clamp_f32(int64_t n, const float* in, float* out, double clamp, ebos_stream_t stream) {
  return clamp_copy<float>("ebos_flow_voxel_clamp_f32", n, in, out, clamp, stream);
}
int ebos_flow_voxel_clamp_f64(int64_t n, const double* in, double* out, double clamp, ebos_stream_t stream) {
  return clamp_copy<double>("ebos_flow_voxel_clamp_f64", n, in, out, clamp, stream);
}

}  // extern "C"
