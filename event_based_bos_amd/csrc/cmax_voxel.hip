// cmax_voxel.hip -- the Adam loop of the time-aware patch-flow contrast maximisation, enqueued by one C call
// (ebos_cmax_voxel_solve_f32): theta -> dense flow at t0 -> flow voxel -> time-aware IWE -> variance [+ flow regularisers]
// -> d_voxel (pixel-owner backward, warp_voxel.hip) -> adjoint of the voxel -> adjoint of the upsample + Adam.  Every stage is an
// entry point of the library; the one kernel here adds the regularisers' gradient to d_dense.
// ebos_cmax_voxel_solve_batch_f32 is the same loop for B windows of one geometry: every stage is called once for all of them, the
// window being an outer grid dimension of its kernel.
#include "common.h"

namespace ebos {
namespace {

__global__ void __launch_bounds__(256) add_inplace_kernel(float* __restrict__ acc, const float* __restrict__ add, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc[i] += add[i];
}

bool has_reg(const ebos_cmax_voxel_problem* q) { return q->w_flow_norm != 0.0f || q->w_image_gradient != 0.0f; }

bool tiled_forward(const ebos_cmax_voxel_problem* q) {
  if (q->halo <= 0) return false;
  int cfg[3 * 64];
  const int n = ebos_tiled_config(cfg, 64);
  for (int i = 0; i < n && i < 64; ++i)
    if (cfg[3 * i] == q->tile_h && cfg[3 * i + 1] == q->tile_w && cfg[3 * i + 2] == q->halo) return true;
  return false;
}

int check_problem(const ebos_cmax_voxel_problem* q) {
  EBOS_REQUIRE(q != nullptr, "ebos_cmax_voxel_solve: NULL problem");
  EBOS_REQUIRE(q->steps_done >= 0, "ebos_cmax_voxel_solve: negative steps_done");
  EBOS_REQUIRE(q->T >= 1 && q->T <= 255, "ebos_cmax_voxel_solve: T = %d is outside [1, 255]", q->T);
  EBOS_REQUIRE(q->scheme == EBOS_FLOW_UPWIND || q->scheme == EBOS_FLOW_BURGERS,
               "ebos_cmax_voxel_solve: scheme %d is neither EBOS_FLOW_UPWIND nor EBOS_FLOW_BURGERS", q->scheme);
  EBOS_REQUIRE(q->theta && q->d_theta && q->exp_avg && q->exp_avg_sq && q->step, "ebos_cmax_voxel_solve: NULL theta / d_theta / Adam state");
  EBOS_REQUIRE(q->key_offsets && ((q->xs && q->ys && q->dts && q->bins) || q->n == 0), "ebos_cmax_voxel_solve: NULL plan buffer");
  EBOS_REQUIRE(q->dense && q->d_dense && q->voxel && q->d_voxel && q->iwe && q->variance && q->moments && q->upstream && q->affine &&
                   q->cost_scratch && q->reg_partials && q->upsample_scratch,
               "ebos_cmax_voxel_solve: NULL image / scratch buffer");
  EBOS_REQUIRE(!q->has_clamp || (q->voxel_clamped && q->clamp == q->clamp), "ebos_cmax_voxel_solve: has_clamp needs voxel_clamped and a number");
  EBOS_REQUIRE(!has_reg(q) || q->d_reg, "ebos_cmax_voxel_solve: regulariser weights given but d_reg is NULL");
  EBOS_REQUIRE(q->w_variance != 0.0f, "ebos_cmax_voxel_solve: w_variance must be non-zero");
  EBOS_REQUIRE(q->n >= 0 && q->n <= INT32_MAX && q->H > 0 && q->W > 0 && q->tile_h > 0 && q->tile_w > 0 && q->pad_h >= 0 && q->pad_w >= 0 &&
                   q->splits >= 1 && q->splits <= 64 && q->gh >= 1 && q->gw >= 1 && q->losses_cap >= 0,
               "ebos_cmax_voxel_solve: bad sizes");
  EBOS_REQUIRE(q->t0_index >= 0 && q->t0_index < q->T, "ebos_cmax_voxel_solve: t0_index %d is outside the %d bins", q->t0_index, q->T);
  EBOS_REQUIRE(q->owner_bwd == 0 || q->owner_bwd == 1, "ebos_cmax_voxel_solve: owner_bwd is 0 or 1");
  const int64_t need = ebos_flow_voxel_advect_adjoint_workspace(q->scheme, 1, q->T, q->H, q->W, q->t0_index, q->wrap_last, q->route);
  if (need < 0) return EBOS_ERR_INVALID_ARG;  // (ebos_last_error: the adjoint's own message)
  if (need > 0 && (q->adjoint_workspace == nullptr || q->adjoint_workspace_elems < need)) {
    set_error("ebos_cmax_voxel_solve: adjoint_workspace holds %lld floats, the voxel's adjoint needs %lld",
              (long long)(q->adjoint_workspace ? q->adjoint_workspace_elems : 0), (long long)need);
    return EBOS_ERR_SCRATCH;
  }
  if (q->cost_scratch_bytes < ebos_cost_scratch_bytes(1)) {
    set_error("ebos_cmax_voxel_solve: cost_scratch too small (%zu < %zu)", q->cost_scratch_bytes, ebos_cost_scratch_bytes(1));
    return EBOS_ERR_SCRATCH;
  }
  return EBOS_OK;
}

// theta -> ... -> d_dense (steps 1 to 7 of an iteration); variance and reg_partials hold the value's two parts
int forward_backward(const ebos_cmax_voxel_problem* q, bool tiled, ebos_stream_t stream) {
  const int H = q->H, W = q->W, T = q->T, h = H + 2 * q->pad_h, w = W + 2 * q->pad_w;
  const int64_t cells = (int64_t)T * 2 * H * W;
  int rc = ebos_upsample_patch_flow_f32(q->theta, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, H, W, q->dense, stream);
  if (rc) return rc;
  // the chain's steps run on unclamped values, and the adjoint reads them: the clamp is a copy of its own
  rc = ebos_flow_voxel_advect_f32(q->scheme, 1, T, H, W, q->dense, q->voxel, q->t0_index, 0, 0.0, q->wrap_last, q->route, stream);
  if (rc) return rc;
  const float* vox = q->voxel;
  if (q->has_clamp) {
    rc = ebos_flow_voxel_clamp_f32(cells, q->voxel, q->voxel_clamped, q->clamp, stream);
    if (rc) return rc;
    vox = q->voxel_clamped;
  }
  if (hipMemsetAsync(q->iwe, 0, (size_t)h * w * sizeof(float), as_stream(stream)) != hipSuccess) {
    set_error("ebos_cmax_voxel_solve: clearing the IWE failed");
    return EBOS_ERR_LAUNCH;
  }
  if (tiled)
    rc = ebos_iwe_voxel_tiled_f32(q->xs, q->ys, q->dts, nullptr, q->bins, q->key_offsets, q->n, vox, T, H, W, q->tile_h, q->tile_w, q->halo,
                                  q->splits, q->pad_h, q->pad_w, q->iwe, stream);
  else
    rc = ebos_iwe_voxel_f32(q->xs, q->ys, q->dts, nullptr, q->bins, q->n, vox, T, H, W, W, q->pad_h, q->pad_w, q->iwe, stream);
  if (rc) return rc;
  rc = ebos_image_variance_f32(q->iwe, 1, h, w, q->omit_boundary, q->variance, q->moments, q->cost_scratch, q->cost_scratch_bytes, stream);
  if (rc) return rc;
  rc = ebos_image_variance_affine_f32(q->moments, q->upstream, 1, q->affine, stream);
  if (rc) return rc;
  if (has_reg(q)) {
    rc = ebos_flow_regularisers_f32(q->dense, H, W, q->w_flow_norm, q->w_image_gradient, q->d_reg, q->reg_partials, nullptr, 0, 0, nullptr,
                                    nullptr, stream);
    if (rc) return rc;
  }
  const int g_lo = q->omit_boundary ? 1 : 0;
  if (q->owner_bwd) {
    rc = ebos_iwe_voxel_owner_bwd_f32(q->xs, q->ys, q->dts, nullptr, q->bins, q->key_offsets, q->n, vox, T, H, W, q->tile_h, q->tile_w,
                                      q->pad_h, q->pad_w, q->iwe, q->affine, g_lo, q->d_voxel, stream);
  } else {
    if (hipMemsetAsync(q->d_voxel, 0, (size_t)cells * sizeof(float), as_stream(stream)) != hipSuccess) {
      set_error("ebos_cmax_voxel_solve: clearing d_voxel failed");
      return EBOS_ERR_LAUNCH;
    }
    rc = ebos_iwe_voxel_bwd_f32(q->xs, q->ys, q->dts, nullptr, q->bins, q->n, vox, T, H, W, W, q->pad_h, q->pad_w, q->iwe, q->affine, g_lo, 1,
                                q->d_voxel, nullptr, stream);
  }
  if (rc) return rc;
  rc = ebos_flow_voxel_advect_adjoint_f32(q->scheme, 1, T, H, W, q->dense, q->voxel, q->d_voxel, q->d_dense, q->t0_index, q->has_clamp, q->clamp,
                                          q->wrap_last, q->route, q->adjoint_workspace, stream);
  if (rc) return rc;
  if (has_reg(q)) {  // added to the flow's gradient itself: through grad_voxel[t0] the clamp's mask would touch it
    const int64_t n = 2 * (int64_t)H * W;
    add_inplace_kernel<<<dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream)>>>(q->d_dense, q->d_reg, n);
    EBOS_CHECK_LAUNCH("ebos_cmax_voxel_solve (regulariser gradient)");
  }
  return EBOS_OK;
}

// ---- several windows per call ---------------------------------------------------------------------
bool has_reg(const ebos_cmax_voxel_batch_problem* q) { return q->w_flow_norm != 0.0f || q->w_image_gradient != 0.0f; }

bool tiled_forward(const ebos_cmax_voxel_batch_problem* q) {
  ebos_cmax_voxel_problem one{};
  one.tile_h = q->tile_h, one.tile_w = q->tile_w, one.halo = q->halo;
  return tiled_forward(&one);
}

int check_batch_problem(const ebos_cmax_voxel_batch_problem* q) {
  EBOS_REQUIRE(q != nullptr, "ebos_cmax_voxel_solve_batch: NULL problem");
  EBOS_REQUIRE(q->B >= 1 && q->B <= EBOS_CMAX_VOXEL_MAX_BATCH, "ebos_cmax_voxel_solve_batch: B = %d is outside [1, %d]", q->B,
               EBOS_CMAX_VOXEL_MAX_BATCH);
  EBOS_REQUIRE(q->steps_done >= 0, "ebos_cmax_voxel_solve_batch: negative steps_done");
  EBOS_REQUIRE(q->T >= 1 && q->T <= 255, "ebos_cmax_voxel_solve_batch: T = %d is outside [1, 255]", q->T);
  EBOS_REQUIRE(q->scheme == EBOS_FLOW_UPWIND || q->scheme == EBOS_FLOW_BURGERS,
               "ebos_cmax_voxel_solve_batch: scheme %d is neither EBOS_FLOW_UPWIND nor EBOS_FLOW_BURGERS", q->scheme);
  EBOS_REQUIRE(q->theta && q->d_theta && q->exp_avg && q->exp_avg_sq && q->step,
               "ebos_cmax_voxel_solve_batch: NULL theta / d_theta / Adam state");
  int64_t total = 0;
  for (int b = 0; b < q->B; ++b) {
    EBOS_REQUIRE(q->n[b] >= 0, "ebos_cmax_voxel_solve_batch: window %d has n = %lld", b, (long long)q->n[b]);
    total += q->n[b];
    EBOS_REQUIRE(total <= INT32_MAX, "ebos_cmax_voxel_solve_batch: the windows hold more than INT32_MAX events");
  }
  EBOS_REQUIRE(q->key_offsets && ((q->xs && q->ys && q->dts && q->bins) || total == 0), "ebos_cmax_voxel_solve_batch: NULL plan buffer");
  EBOS_REQUIRE(q->dense && q->d_dense && q->voxel && q->d_voxel && q->iwe && q->variance && q->moments && q->upstream && q->affine &&
                   q->cost_scratch && q->reg_partials && q->upsample_scratch,
               "ebos_cmax_voxel_solve_batch: NULL image / scratch buffer");
  EBOS_REQUIRE(!q->has_clamp || (q->voxel_clamped && q->clamp == q->clamp),
               "ebos_cmax_voxel_solve_batch: has_clamp needs voxel_clamped and a number");
  EBOS_REQUIRE(!has_reg(q) || q->d_reg, "ebos_cmax_voxel_solve_batch: regulariser weights given but d_reg is NULL");
  EBOS_REQUIRE(q->w_variance != 0.0f, "ebos_cmax_voxel_solve_batch: w_variance must be non-zero");
  EBOS_REQUIRE(q->H > 0 && q->W > 0 && q->tile_h > 0 && q->tile_w > 0 && q->pad_h >= 0 && q->pad_w >= 0 && q->splits >= 1 &&
                   q->splits <= 64 && q->gh >= 1 && q->gw >= 1 && q->losses_cap >= 0,
               "ebos_cmax_voxel_solve_batch: bad sizes");
  EBOS_REQUIRE(q->t0_index >= 0 && q->t0_index < q->T, "ebos_cmax_voxel_solve_batch: t0_index %d is outside the %d bins", q->t0_index, q->T);
  EBOS_REQUIRE(q->owner_bwd == 0 || q->owner_bwd == 1, "ebos_cmax_voxel_solve_batch: owner_bwd is 0 or 1");
  const int64_t need = ebos_flow_voxel_advect_adjoint_workspace(q->scheme, q->B, q->T, q->H, q->W, q->t0_index, q->wrap_last, q->route);
  if (need < 0) return EBOS_ERR_INVALID_ARG;  // (ebos_last_error: the adjoint's own message)
  if (need > 0 && (q->adjoint_workspace == nullptr || q->adjoint_workspace_elems < need)) {
    set_error("ebos_cmax_voxel_solve_batch: adjoint_workspace holds %lld floats, the adjoint of %d voxels needs %lld",
              (long long)(q->adjoint_workspace ? q->adjoint_workspace_elems : 0), q->B, (long long)need);
    return EBOS_ERR_SCRATCH;
  }
  if (q->cost_scratch_bytes < ebos_cost_scratch_bytes(q->B)) {
    set_error("ebos_cmax_voxel_solve_batch: cost_scratch too small for %d windows (%zu < %zu)", q->B, q->cost_scratch_bytes,
              ebos_cost_scratch_bytes(q->B));
    return EBOS_ERR_SCRATCH;
  }
  return EBOS_OK;
}

// forward_backward with every stage called once for the B windows
int forward_backward_batch(const ebos_cmax_voxel_batch_problem* q, bool tiled, ebos_stream_t stream) {
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
  if (hipMemsetAsync(q->iwe, 0, (size_t)B * h * w * sizeof(float), as_stream(stream)) != hipSuccess) {
    set_error("ebos_cmax_voxel_solve_batch: clearing the IWEs failed");
    return EBOS_ERR_LAUNCH;
  }
  // (halo <= 0 names no built configuration: the entry point falls back to the general kernel window by window)
  rc = ebos_iwe_voxel_tiled_batch_f32(q->xs, q->ys, q->dts, q->bins, q->key_offsets, q->n, B, vox, T, H, W, q->tile_h, q->tile_w,
                                      tiled ? q->halo : 0, q->splits, q->pad_h, q->pad_w, q->iwe, stream);
  if (rc) return rc;
  rc = ebos_image_variance_f32(q->iwe, B, h, w, q->omit_boundary, q->variance, q->moments, q->cost_scratch, q->cost_scratch_bytes, stream);
  if (rc) return rc;
  rc = ebos_image_variance_affine_f32(q->moments, q->upstream, B, q->affine, stream);
  if (rc) return rc;
  if (has_reg(q)) {
    rc = ebos_flow_regularisers_batch_f32(q->dense, B, H, W, q->w_flow_norm, q->w_image_gradient, q->d_reg, q->reg_partials, stream);
    if (rc) return rc;
  }
  const int g_lo = q->omit_boundary ? 1 : 0;
  if (q->owner_bwd) {
    rc = ebos_iwe_voxel_owner_bwd_batch_f32(q->xs, q->ys, q->dts, q->bins, q->key_offsets, q->n, B, vox, T, H, W, q->tile_h, q->tile_w,
                                            q->pad_h, q->pad_w, q->iwe, q->affine, g_lo, q->d_voxel, stream);
    if (rc) return rc;
  } else {
    if (hipMemsetAsync(q->d_voxel, 0, (size_t)B * cells * sizeof(float), as_stream(stream)) != hipSuccess) {
      set_error("ebos_cmax_voxel_solve_batch: clearing d_voxel failed");
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
    EBOS_CHECK_LAUNCH("ebos_cmax_voxel_solve_batch (regulariser gradient)");
  }
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

int ebos_cmax_voxel_solve_f32(const ebos_cmax_voxel_problem* q, int n_iter, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(n_iter >= 0, "ebos_cmax_voxel_solve: negative n_iter");
  if (int rc = check_problem(q)) return rc;
  const bool tiled = tiled_forward(q);
  const int n_reg = has_reg(q) ? ebos_flow_regularisers_partials() : 0;
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = forward_backward(q, tiled, stream)) return rc;
    // adjoint of the upsample + the Adam step of every grid element where its gradient appears + the loss of the iteration
    if (int rc = ebos_upsample_patch_flow_bwd_adam_f32(q->d_dense, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, q->H, q->W,
                                                       q->upsample_scratch, q->d_theta, q->theta, q->exp_avg, q->exp_avg_sq, q->lr, q->beta1,
                                                       q->beta2, q->eps, q->steps_done + it + 1, q->step, q->variance, -q->w_variance,
                                                       q->reg_partials, n_reg, q->losses, q->losses_cap, q->theta_mask, stream))
      return rc;
  }
  return EBOS_OK;
}

int ebos_cmax_voxel_gradient_f32(const ebos_cmax_voxel_problem* q, ebos_stream_t stream) {
  using namespace ebos;
  if (int rc = check_problem(q)) return rc;
  if (int rc = forward_backward(q, tiled_forward(q), stream)) return rc;
  return ebos_upsample_patch_flow_bwd_f32(q->d_dense, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, q->H, q->W,
                                          q->upsample_scratch, q->d_theta, stream);
}

int ebos_cmax_voxel_solve_batch_f32(const ebos_cmax_voxel_batch_problem* q, int n_iter, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(n_iter >= 0, "ebos_cmax_voxel_solve_batch: negative n_iter");
  if (int rc = check_batch_problem(q)) return rc;
  const bool tiled = tiled_forward(q);
  const int n_reg = has_reg(q) ? ebos_flow_regularisers_partials() : 0;
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = forward_backward_batch(q, tiled, stream)) return rc;
    if (int rc = ebos_upsample_patch_flow_bwd_adam_batch_f32(
            q->d_dense, q->B, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, q->H, q->W, q->upsample_scratch, q->d_theta,
            q->theta, q->exp_avg, q->exp_avg_sq, q->lr, q->beta1, q->beta2, q->eps, q->steps_done + it + 1, q->step, q->variance,
            -q->w_variance, q->reg_partials, n_reg, q->losses, q->losses_cap, q->theta_mask, stream))
      return rc;
  }
  return EBOS_OK;
}

int ebos_cmax_voxel_gradient_batch_f32(const ebos_cmax_voxel_batch_problem* q, ebos_stream_t stream) {
  using namespace ebos;
  if (int rc = check_batch_problem(q)) return rc;
  if (int rc = forward_backward_batch(q, tiled_forward(q), stream)) return rc;
  return ebos_upsample_patch_flow_bwd_batch_f32(q->d_dense, q->B, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, q->H, q->W,
                                                q->upsample_scratch, q->d_theta, stream);
}

}  // extern "C"
