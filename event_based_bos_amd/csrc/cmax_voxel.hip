// cmax_voxel.hip -- the Adam loop of the time-aware patch-flow contrast maximisation for B windows of one geometry, enqueued by one
// C call (ebos_cmax_voxel_solve_batch_f32): theta -> dense flow at t0 -> flow voxel -> time-aware IWE -> variance [+ flow regularisers]
// -> d_voxel (pixel-owner backward, warp_voxel.hip) -> adjoint of the voxel -> adjoint of the upsample + Adam.  Every stage is a
// `_batch_` entry point of the library, called once for all windows, the window being an outer grid dimension of its kernel; the one
// kernel here adds the regularisers' gradient to d_dense.
// One window is a batch of one: ebos_cmax_voxel_solve_f32 / _gradient_f32 copy their problem into a batch problem with B = 1 and run
// this same code.
// K reference times (ebos_cmax_voxel_multiref_solve_batch_f32): the same stages on B K images -- the forward and the owner backward of
// warp_voxel_multiref.hip in the place of the single reference's, and one small kernel that folds a window's K variances into its
// value; the problem is copied into a batch problem plus a `MultiRef` and runs this same code too.
#include <cmath>

#include "common.h"
#include "tile_configs.h"

namespace ebos {
namespace {

__global__ void __launch_bounds__(256) add_inplace_kernel(float* __restrict__ acc, const float* __restrict__ add, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc[i] += add[i];
}

// value[b] = inv_norm[b] * mean_k variance[b][k]: what the Adam kernel records as window b's contrast
__global__ void __launch_bounds__(64) multiref_value_kernel(const float* __restrict__ variance, const float* __restrict__ inv_norm, int B,
                                                            int K, float* __restrict__ value) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double sum = 0.0;
  for (int k = 0; k < K; ++k) sum += (double)variance[b * K + k];
  value[b] = (float)((double)inv_norm[b] * (sum / K));
}

// what K reference times add to a batch problem (nullptr: one reference time, the plan's own)
struct MultiRef {
  int K;
  const float* shifts;    // [K], host
  const float* inv_norm;  // [B], device
  float* value;           // [B], device
};

bool has_reg(const ebos_cmax_voxel_batch_problem* q) { return q->w_flow_norm != 0.0f || q->w_image_gradient != 0.0f; }

bool tiled_forward(const ebos_cmax_voxel_batch_problem* q) {
  return q->halo > 0 && config_ok(kTiledConfigs, q->tile_h, q->tile_w, q->halo);
}

// `who`: the entry point the caller used, in front of every refusal
// `n_ref`: images per window (the cost kernels' scratch holds B * n_ref of them)
int check_problem(const char* who, const ebos_cmax_voxel_batch_problem* q, int n_ref = 1) {
  EBOS_REQUIRE(q != nullptr, "%s: NULL problem", who);
  EBOS_REQUIRE(q->B >= 1 && q->B <= EBOS_CMAX_VOXEL_MAX_BATCH, "%s: B = %d is outside [1, %d]", who, q->B,
               EBOS_CMAX_VOXEL_MAX_BATCH);
  EBOS_REQUIRE(q->steps_done >= 0, "%s: negative steps_done", who);
  EBOS_REQUIRE(q->T >= 1 && q->T <= 255, "%s: T = %d is outside [1, 255]", who, q->T);
  EBOS_REQUIRE(q->scheme == EBOS_FLOW_UPWIND || q->scheme == EBOS_FLOW_BURGERS,
               "%s: scheme %d is neither EBOS_FLOW_UPWIND nor EBOS_FLOW_BURGERS", who, q->scheme);
  EBOS_REQUIRE(q->theta && q->d_theta && q->exp_avg && q->exp_avg_sq && q->step,
               "%s: NULL theta / d_theta / Adam state", who);
  int64_t total = 0;
  for (int b = 0; b < q->B; ++b) {
    EBOS_REQUIRE(q->n[b] >= 0, "%s: window %d has n = %lld", who, b, (long long)q->n[b]);
    total += q->n[b];
    EBOS_REQUIRE(total <= INT32_MAX, "%s: the windows hold more than INT32_MAX events", who);
  }
  EBOS_REQUIRE(q->key_offsets && ((q->xs && q->ys && q->dts && q->bins) || total == 0), "%s: NULL plan buffer", who);
  EBOS_REQUIRE(q->dense && q->d_dense && q->voxel && q->d_voxel && q->iwe && q->variance && q->moments && q->upstream && q->affine &&
                   q->cost_scratch && q->reg_partials && q->upsample_scratch,
               "%s: NULL image / scratch buffer", who);
  EBOS_REQUIRE(!q->has_clamp || (q->voxel_clamped && q->clamp == q->clamp),
               "%s: has_clamp needs voxel_clamped and a number", who);
  EBOS_REQUIRE(!has_reg(q) || q->d_reg, "%s: regulariser weights given but d_reg is NULL", who);
  EBOS_REQUIRE(q->w_variance != 0.0f, "%s: w_variance must be non-zero", who);
  EBOS_REQUIRE(q->H > 0 && q->W > 0 && q->tile_h > 0 && q->tile_w > 0 && q->pad_h >= 0 && q->pad_w >= 0 && q->splits >= 1 &&
                   q->splits <= 64 && q->gh >= 1 && q->gw >= 1 && q->losses_cap >= 0,
               "%s: bad sizes", who);
  EBOS_REQUIRE(q->t0_index >= 0 && q->t0_index < q->T, "%s: t0_index %d is outside the %d bins", who, q->t0_index, q->T);
  EBOS_REQUIRE(q->owner_bwd == 0 || q->owner_bwd == 1, "%s: owner_bwd is 0 or 1", who);
  const int64_t need = ebos_flow_voxel_advect_adjoint_workspace(q->scheme, q->B, q->T, q->H, q->W, q->t0_index, q->wrap_last, q->route);
  if (need < 0) return EBOS_ERR_INVALID_ARG;  // (ebos_last_error: the adjoint's own message)
  if (need > 0 && (q->adjoint_workspace == nullptr || q->adjoint_workspace_elems < need)) {
    set_error("%s: adjoint_workspace holds %lld floats, the adjoint of %d voxels needs %lld", who,
              (long long)(q->adjoint_workspace ? q->adjoint_workspace_elems : 0), q->B, (long long)need);
    return EBOS_ERR_SCRATCH;
  }
  if (q->cost_scratch_bytes < ebos_cost_scratch_bytes(q->B * n_ref)) {
    if (n_ref == 1)
      set_error("%s: cost_scratch too small for %d windows (%zu < %zu)", who, q->B, q->cost_scratch_bytes,
                ebos_cost_scratch_bytes(q->B));
    else
      set_error("%s: cost_scratch too small for %d windows x %d reference times (%zu < %zu)", who, q->B, n_ref, q->cost_scratch_bytes,
                ebos_cost_scratch_bytes(q->B * n_ref));
    return EBOS_ERR_SCRATCH;
  }
  return EBOS_OK;
}

// theta -> ... -> d_dense (steps 1 to 7 of an iteration), every stage called once for the B windows; variance and reg_partials hold
// the value's two parts.  With `mr` the images are [B, K, h, w] (variance, moments, upstream and affine hold B K entries, window-major)
// and mr->value receives the windows' values.
int forward_backward(const char* who, const ebos_cmax_voxel_batch_problem* q, bool tiled, ebos_stream_t stream,
                     const MultiRef* mr = nullptr) {
  const int n_img = q->B * (mr ? mr->K : 1);
  const int B = q->B, H = q->H, W = q->W, T = q->T, h = H + 2 * q->pad_h, w = W + 2 * q->pad_w;
  const int64_t cells = (int64_t)T * 2 * H * W;
  int rc = ebos_upsample_patch_flow_batch_f32(q->theta, B, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, H, W, q->dense,
                                              stream);
  if (rc) return rc;
  rc = ebos_flow_voxel_advect_f32(q->scheme, B, T, H, W, q->dense, q->voxel, q->t0_index, 0, 0.0, q->wrap_last, q->route, stream);
  if (rc) return rc;
  const float* vox = q->voxel;
  if (q->has_clamp) {
    rc = ebos_flow_voxel_clamp_f32(B * cells, q->voxel, q->voxel_clamped, q->clamp, stream);
    if (rc) return rc;
    vox = q->voxel_clamped;
  }
  if (hipMemsetAsync(q->iwe, 0, (size_t)n_img * h * w * sizeof(float), as_stream(stream)) != hipSuccess) {
    set_error("%s: clearing the IWEs failed", who);
    return EBOS_ERR_LAUNCH;
  }
  // (halo <= 0 names no built configuration: the entry point falls back to the general kernel window by window)
  if (mr)
    rc = ebos_iwe_voxel_multiref_tiled_batch_f32(q->xs, q->ys, q->dts, q->bins, q->key_offsets, q->n, B, vox, T, H, W, q->tile_h, q->tile_w,
                                                 tiled ? q->halo : 0, q->splits, q->pad_h, q->pad_w, mr->shifts, mr->K, q->iwe, stream);
  else
    rc = ebos_iwe_voxel_tiled_batch_f32(q->xs, q->ys, q->dts, q->bins, q->key_offsets, q->n, B, vox, T, H, W, q->tile_h, q->tile_w,
                                        tiled ? q->halo : 0, q->splits, q->pad_h, q->pad_w, q->iwe, stream);
  if (rc) return rc;
  rc = ebos_image_variance_f32(q->iwe, n_img, h, w, q->omit_boundary, q->variance, q->moments, q->cost_scratch, q->cost_scratch_bytes,
                               stream);
  if (rc) return rc;
  rc = ebos_image_variance_affine_f32(q->moments, q->upstream, n_img, q->affine, stream);
  if (rc) return rc;
  if (mr) {
    multiref_value_kernel<<<dim3((B + 63) / 64), dim3(64), 0, as_stream(stream)>>>(q->variance, mr->inv_norm, B, mr->K, mr->value);
    EBOS_CHECK_LAUNCH(who);  // (the windows' values)
  }
  if (has_reg(q)) {
    rc = ebos_flow_regularisers_batch_f32(q->dense, B, H, W, q->w_flow_norm, q->w_image_gradient, q->d_reg, q->reg_partials, stream);
    if (rc) return rc;
  }
  const int g_lo = q->omit_boundary ? 1 : 0;
  if (mr) {
    rc = ebos_iwe_voxel_multiref_owner_bwd_batch_f32(q->xs, q->ys, q->dts, q->bins, q->key_offsets, q->n, B, vox, T, H, W, q->tile_h,
                                                     q->tile_w, q->pad_h, q->pad_w, mr->shifts, mr->K, q->iwe, q->affine, g_lo, q->d_voxel,
                                                     stream);
    if (rc) return rc;
  } else if (q->owner_bwd) {
    rc = ebos_iwe_voxel_owner_bwd_batch_f32(q->xs, q->ys, q->dts, q->bins, q->key_offsets, q->n, B, vox, T, H, W, q->tile_h, q->tile_w,
                                            q->pad_h, q->pad_w, q->iwe, q->affine, g_lo, q->d_voxel, stream);
    if (rc) return rc;
  } else {
    if (hipMemsetAsync(q->d_voxel, 0, (size_t)B * cells * sizeof(float), as_stream(stream)) != hipSuccess) {
      set_error("%s: clearing d_voxel failed", who);
      return EBOS_ERR_LAUNCH;
    }
    int64_t at = 0;
    for (int b = 0; b < B; ++b) {  // the atomic backward stays a launch per window
      rc = ebos_iwe_voxel_bwd_f32(q->xs + at, q->ys + at, q->dts + at, nullptr, q->bins + at, q->n[b], vox + b * cells, T, H, W, W,
                                  q->pad_h, q->pad_w, q->iwe + (int64_t)b * h * w, q->affine + 2 * b, g_lo, 1, q->d_voxel + b * cells,
                                  nullptr, stream);
      if (rc) return rc;
      at += q->n[b];
    }
  }
  rc = ebos_flow_voxel_advect_adjoint_f32(q->scheme, B, T, H, W, q->dense, q->voxel, q->d_voxel, q->d_dense, q->t0_index, q->has_clamp,
                                          q->clamp, q->wrap_last, q->route, q->adjoint_workspace, stream);
  if (rc) return rc;
  if (has_reg(q)) {
    const int64_t n = (int64_t)B * 2 * H * W;
    add_inplace_kernel<<<dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream)>>>(q->d_dense, q->d_reg, n);
    EBOS_CHECK_LAUNCH(who);  // (the regularisers' gradient)
  }
  return EBOS_OK;
}

// the refusals K reference times add, then check_problem's
int check_multiref(const char* who, const ebos_cmax_voxel_batch_problem* q, const MultiRef* mr) {
  if (mr == nullptr) return check_problem(who, q);
  EBOS_REQUIRE(mr->K >= 1 && mr->K <= EBOS_MULTIREF_MAX, "%s: K = %d is outside [1, %d]", who, mr->K, EBOS_MULTIREF_MAX);
  for (int k = 0; k < mr->K; ++k) EBOS_REQUIRE(std::isfinite(mr->shifts[k]), "%s: shifts[%d] is not finite", who, k);
  EBOS_REQUIRE(mr->inv_norm && mr->value, "%s: NULL inv_norm / value", who);
  return check_problem(who, q, mr->K);
}

int solve(const char* who, const ebos_cmax_voxel_batch_problem* q, int n_iter, ebos_stream_t stream, const MultiRef* mr = nullptr) {
  EBOS_REQUIRE(n_iter >= 0, "%s: negative n_iter", who);
  if (int rc = check_multiref(who, q, mr)) return rc;
  const bool tiled = tiled_forward(q);
  const int n_reg = has_reg(q) ? ebos_flow_regularisers_partials() : 0;
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = forward_backward(who, q, tiled, stream, mr)) return rc;
    // adjoint of the upsample + the Adam step of every grid element where its gradient appears + the loss of the iteration
    if (int rc = ebos_upsample_patch_flow_bwd_adam_batch_f32(
            q->d_dense, q->B, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, q->H, q->W, q->upsample_scratch, q->d_theta,
            q->theta, q->exp_avg, q->exp_avg_sq, q->lr, q->beta1, q->beta2, q->eps, q->steps_done + it + 1, q->step,
            mr ? mr->value : q->variance, -q->w_variance, q->reg_partials, n_reg, q->losses, q->losses_cap, q->theta_mask, stream))
      return rc;
  }
  return EBOS_OK;
}

int gradient(const char* who, const ebos_cmax_voxel_batch_problem* q, ebos_stream_t stream, const MultiRef* mr = nullptr) {
  if (int rc = check_multiref(who, q, mr)) return rc;
  if (int rc = forward_backward(who, q, tiled_forward(q), stream, mr)) return rc;
  return ebos_upsample_patch_flow_bwd_batch_f32(q->d_dense, q->B, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, q->H, q->W,
                                                q->upsample_scratch, q->d_theta, stream);
}

// the fields the three problem structs of include/ebos_hip.h share under one name (all but B / n, owner_bwd and what K adds)
#define EBOS_CMAX_VOXEL_SHARED_FIELDS(X)                                                                                          \
  X(xs) X(ys) X(dts) X(bins) X(key_offsets)                                                                                        \
  X(H) X(W) X(tile_h) X(tile_w) X(halo) X(pad_h) X(pad_w)                                                                          \
  X(omit_boundary) X(splits) X(T) X(scheme) X(t0_index) X(wrap_last) X(route)                                                      \
  X(has_clamp) X(clamp) X(gh) X(gw) X(patch_h) X(patch_w)                                                                          \
  X(slide_h) X(slide_w) X(w_variance) X(w_flow_norm) X(w_image_gradient) X(lr)                                                     \
  X(beta1) X(beta2) X(eps) X(theta) X(d_theta) X(exp_avg) X(exp_avg_sq)                                                            \
  X(step) X(steps_done) X(dense) X(d_dense) X(d_reg) X(voxel) X(voxel_clamped)                                                     \
  X(d_voxel) X(iwe) X(variance) X(moments) X(upstream) X(affine) X(cost_scratch)                                                   \
  X(cost_scratch_bytes) X(reg_partials) X(upsample_scratch) X(adjoint_workspace)                                                   \
  X(adjoint_workspace_elems) X(losses) X(losses_cap) X(theta_mask)
#define EBOS_COPY(f) b.f = q->f;

// one window as a batch of one: B = 1, n[0] = n, every other field under its own name
ebos_cmax_voxel_batch_problem batch_of_one(const ebos_cmax_voxel_problem* q) {
  ebos_cmax_voxel_batch_problem b{};
  b.B = 1, b.n[0] = q->n, b.owner_bwd = q->owner_bwd;
  EBOS_CMAX_VOXEL_SHARED_FIELDS(EBOS_COPY)
  return b;
}

// K reference times: the batch problem under the same field names (the owner backward is the only one), and what K adds
ebos_cmax_voxel_batch_problem batch_of_multiref(const ebos_cmax_voxel_multiref_batch_problem* q, MultiRef* mr) {
  ebos_cmax_voxel_batch_problem b{};
  b.B = q->B, b.owner_bwd = 1;
  for (int i = 0; i < EBOS_CMAX_VOXEL_MAX_BATCH; ++i) b.n[i] = q->n[i];
  EBOS_CMAX_VOXEL_SHARED_FIELDS(EBOS_COPY)
  mr->K = q->K, mr->shifts = q->shifts, mr->inv_norm = q->inv_norm, mr->value = q->value;
  return b;
}
#undef EBOS_COPY
#undef EBOS_CMAX_VOXEL_SHARED_FIELDS

}  // namespace
}  // namespace ebos

extern "C" {

int ebos_cmax_voxel_solve_batch_f32(const ebos_cmax_voxel_batch_problem* q, int n_iter, ebos_stream_t stream) {
  return ebos::solve("ebos_cmax_voxel_solve_batch", q, n_iter, stream);
}

int ebos_cmax_voxel_gradient_batch_f32(const ebos_cmax_voxel_batch_problem* q, ebos_stream_t stream) {
  return ebos::gradient("ebos_cmax_voxel_gradient_batch", q, stream);
}

int ebos_cmax_voxel_solve_f32(const ebos_cmax_voxel_problem* q, int n_iter, ebos_stream_t stream) {
  EBOS_REQUIRE(q != nullptr, "ebos_cmax_voxel_solve: NULL problem");
  const ebos_cmax_voxel_batch_problem one = ebos::batch_of_one(q);
  return ebos::solve("ebos_cmax_voxel_solve", &one, n_iter, stream);
}

int ebos_cmax_voxel_gradient_f32(const ebos_cmax_voxel_problem* q, ebos_stream_t stream) {
  EBOS_REQUIRE(q != nullptr, "ebos_cmax_voxel_gradient: NULL problem");
  const ebos_cmax_voxel_batch_problem one = ebos::batch_of_one(q);
  return ebos::gradient("ebos_cmax_voxel_gradient", &one, stream);
}

int ebos_cmax_voxel_multiref_solve_batch_f32(const ebos_cmax_voxel_multiref_batch_problem* q, int n_iter, ebos_stream_t stream) {
  EBOS_REQUIRE(q != nullptr, "ebos_cmax_voxel_multiref_solve_batch: NULL problem");
  ebos::MultiRef mr;
  const ebos_cmax_voxel_batch_problem one = ebos::batch_of_multiref(q, &mr);
  return ebos::solve("ebos_cmax_voxel_multiref_solve_batch", &one, n_iter, stream, &mr);
}

int ebos_cmax_voxel_multiref_gradient_batch_f32(const ebos_cmax_voxel_multiref_batch_problem* q, ebos_stream_t stream) {
  EBOS_REQUIRE(q != nullptr, "ebos_cmax_voxel_multiref_gradient_batch: NULL problem");
  ebos::MultiRef mr;
  const ebos_cmax_voxel_batch_problem one = ebos::batch_of_multiref(q, &mr);
  return ebos::gradient("ebos_cmax_voxel_multiref_gradient_batch", &one, stream, &mr);
}

}  // extern "C"
