// cmax_multiref.hip -- the Adam loop of the multi-reference patch-flow contrast maximisation (the solver's `multi_reference` block
// with `native: true`), enqueued by one C call (ebos_cmax_multiref_solve_f32):
//
//     loss(theta) = -(w_variance / (K N)) sum_k var(IWE_k(dense(theta))) + w_flow_norm flow_norm(dense) + w_image_gradient TV(dense)
//
// One iteration, every stage an entry point of the library:
//     ebos_upsample_patch_flow_f32               1 launch    theta -> dense
//     ebos_iwe_dense_slab_multiref_f32           2 launches  accumulate over (work item, k), combine over (pixel block, k): K IWEs, K variances
//     ebos_flow_regularisers_f32                 1 launch    (only with a regulariser weight) value partials + gradient image
//     ebos_iwe_dense_tiled_multiref_bwd_f32      1 launch    d_dense = sum over the references, + the regularisers' gradient
//     multiref_fold_kernel (here)                1 launch    contrast = sum_k variance_k, the one scalar the Adam step kernel reads
//     ebos_upsample_patch_flow_bwd_adam_f32      2 launches  d_theta, the Adam step, losses[step]
// 7 launches per iteration, 8 with regularisers -- whatever K is.
#include "common.h"

namespace ebos {
namespace {

__global__ void __launch_bounds__(64) multiref_fold_kernel(const float* __restrict__ variances, int K, float* __restrict__ contrast) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float s = 0.0f;
    for (int k = 0; k < K; ++k) s += variances[k];  // reference order: the same bits on every call
    contrast[0] = s;
  }
}

bool has_reg(const ebos_cmax_multiref_problem* q) { return q->w_flow_norm != 0.0f || q->w_image_gradient != 0.0f; }

float contrast_scale(const ebos_cmax_multiref_problem* q) { return (float)(-(double)q->w_variance / ((double)q->K * q->norm)); }

int check_problem(const char* who, const ebos_cmax_multiref_problem* q) {
  EBOS_REQUIRE(q != nullptr, "%s: NULL problem", who);
  EBOS_REQUIRE(q->K >= 1 && q->K <= EBOS_MULTIREF_MAX, "%s: K = %d is outside [1, %d]", who, q->K, EBOS_MULTIREF_MAX);
  for (int k = 0; k < q->K; ++k) EBOS_REQUIRE(q->shifts[k] == q->shifts[k] && q->shifts[k] - q->shifts[k] == 0.0f, "%s: shifts[%d] is not finite", who, k);
  EBOS_REQUIRE(q->steps_done >= 0, "%s: negative steps_done", who);
  EBOS_REQUIRE(q->theta && q->d_theta && q->exp_avg && q->exp_avg_sq && q->step, "%s: NULL theta / d_theta / Adam state", who);
  EBOS_REQUIRE(q->key_offsets && ((q->xs && q->ys && q->dts) || q->n == 0), "%s: NULL plan buffer", who);
  EBOS_REQUIRE(q->dense && q->d_dense && q->iwes && q->variances && q->moments && q->contrast && q->upstream && q->workspace &&
                   q->reg_partials && q->upsample_scratch,
               "%s: NULL image / scratch buffer", who);
  EBOS_REQUIRE(!has_reg(q) || q->d_reg, "%s: regulariser weights given but d_reg is NULL", who);
  EBOS_REQUIRE(q->w_variance != 0.0f, "%s: w_variance must be non-zero", who);
  EBOS_REQUIRE(q->norm == q->norm && q->norm != 0.0 && q->norm - q->norm == 0.0, "%s: norm (N) must be finite and non-zero", who);
  EBOS_REQUIRE(q->n >= 0 && q->n <= INT32_MAX && q->H > 0 && q->W > 0 && q->tile_h > 0 && q->tile_w > 0 && q->pad_h >= 0 && q->pad_w >= 0 &&
                   q->splits >= 0 && q->splits <= 64 && q->gh >= 1 && q->gw >= 1 && q->losses_cap >= 0,
               "%s: bad sizes", who);
  if (q->splits == 0 || q->halo < 0 ||
      ebos_iwe_slab_multiref_workspace_bytes(q->K, q->H, q->W, q->tile_h, q->tile_w, q->halo, q->splits, q->pad_h, q->pad_w) == 0) {
    set_error("%s: no multi-reference kernel for tile %dx%d halo %d splits %d (ebos_slab_multiref_config lists the built triples; "
              "adaptive work items and run-time windows are not built)", who, q->tile_h, q->tile_w, q->halo, q->splits);
    return EBOS_ERR_UNSUPPORTED;
  }
  const size_t need = ebos_iwe_slab_multiref_workspace_bytes(q->K, q->H, q->W, q->tile_h, q->tile_w, q->halo, q->splits, q->pad_h, q->pad_w);
  if (q->workspace_bytes < need) {
    set_error("%s: workspace too small (%zu < %zu)", who, q->workspace_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  const size_t need_up = ebos_upsample_bwd_scratch_bytes(q->gh, q->W);
  if (q->upsample_scratch_bytes < need_up) {
    set_error("%s: upsample_scratch too small (%zu < %zu)", who, q->upsample_scratch_bytes, need_up);
    return EBOS_ERR_SCRATCH;
  }
  return EBOS_OK;
}

// theta -> ... -> d_dense and the folded contrast; variances and reg_partials hold the value's parts
int forward_backward(const ebos_cmax_multiref_problem* q, ebos_stream_t stream) {
  const int H = q->H, W = q->W;
  int rc = ebos_upsample_patch_flow_f32(q->theta, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, H, W, q->dense, stream);
  if (rc) return rc;
  rc = ebos_iwe_dense_slab_multiref_f32(q->xs, q->ys, q->dts, q->key_offsets, q->n, q->dense, H, W, q->tile_h, q->tile_w, q->halo, q->splits,
                                        q->pad_h, q->pad_w, q->shifts, q->K, q->workspace, q->workspace_bytes, q->iwes, 1, q->omit_boundary,
                                        q->variances, q->moments, stream);
  if (rc) return rc;
  if (has_reg(q)) {
    rc = ebos_flow_regularisers_f32(q->dense, H, W, q->w_flow_norm, q->w_image_gradient, q->d_reg, q->reg_partials, nullptr, 0, 0, nullptr,
                                    nullptr, stream);
    if (rc) return rc;
  }
  rc = ebos_iwe_dense_tiled_multiref_bwd_f32(q->xs, q->ys, q->dts, q->key_offsets, q->n, q->dense, H, W, q->tile_h, q->tile_w, q->halo, q->pad_h,
                                             q->pad_w, q->shifts, q->K, q->iwes, nullptr, q->omit_boundary ? 1 : 0, q->moments, q->upstream,
                                             nullptr, has_reg(q) ? q->d_reg : nullptr, q->d_dense, stream);
  if (rc) return rc;
  multiref_fold_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(q->variances, q->K, q->contrast);
  EBOS_CHECK_LAUNCH("ebos_cmax_multiref (fold)");
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

int ebos_cmax_multiref_solve_f32(const ebos_cmax_multiref_problem* q, int n_iter, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE(n_iter >= 0, "ebos_cmax_multiref_solve: negative n_iter");
  if (int rc = check_problem("ebos_cmax_multiref_solve", q)) return rc;
  const int n_reg = has_reg(q) ? ebos_flow_regularisers_partials() : 0;
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = forward_backward(q, stream)) return rc;
    if (int rc = ebos_upsample_patch_flow_bwd_adam_f32(q->d_dense, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, q->H, q->W,
                                                       q->upsample_scratch, q->d_theta, q->theta, q->exp_avg, q->exp_avg_sq, q->lr, q->beta1,
                                                       q->beta2, q->eps, q->steps_done + it + 1, q->step, q->contrast, contrast_scale(q),
                                                       q->reg_partials, n_reg, q->losses, q->losses_cap, q->theta_mask, stream))
      return rc;
  }
  return EBOS_OK;
}

int ebos_cmax_multiref_gradient_f32(const ebos_cmax_multiref_problem* q, ebos_stream_t stream) {
  using namespace ebos;
  if (int rc = check_problem("ebos_cmax_multiref_gradient", q)) return rc;
  if (int rc = forward_backward(q, stream)) return rc;
  return ebos_upsample_patch_flow_bwd_f32(q->d_dense, q->gh, q->gw, q->patch_h, q->patch_w, q->slide_h, q->slide_w, q->H, q->W,
                                          q->upsample_scratch, q->d_theta, stream);
}

}  // extern "C"
