/*
 * ebos_hip.h -- C ABI of libebos_hip.so: the MI355X (gfx950) implementation of the
 * contrast-maximisation inner loop of event-based BOS
 *        warp events -> bilinear-splat image of warped events (IWE) -> contrast cost (+ gradients)
 *
 * The reference (tub-rip/event_based_bos) is pure Python and has no FFI for this path; its
 * boundary is the plugin surface Warp / EventImageConverter / costs.  Every
 * entry point below names the reference code (file:line under /root/reference) that it replaces.
 * The Python host package event_based_bos_amd binds these symbols with ctypes
 * (INTEGRATION.md shows the stub a maintainer of the reference would add).
 *
 * Conventions
 *  - plain C types only; every pointer is a DEVICE pointer unless it says "host";
 *  - nothing is allocated, freed or synchronised in here: the caller owns every buffer (torch's
 *    caching allocator in practice) and every call is asynchronous on `stream` (a hipStream_t
 *    passed as void*; NULL = the default stream).  All entry points are graph-capturable;
 *  - return value: EBOS_OK (0) or a negative ebos_status; ebos_last_error() gives the message
 *    (thread-local, valid until the next failing call on that thread);
 *  - event = (x, y, t, p) with x = ROW coordinate and y = COLUMN coordinate
 *    (src/data_loader/ccs.py:293-296); images are [H, W] row-major; flow is [2, H, W] with
 *    channel 0 = row displacement (src/warp.py:333-336);
 *  - suffix _f32 / _f64 = element type of events, flow and images.  The *_soa_* hot path is f32.
 *  - "accumulates": the kernel ADDS into the output; the caller zeroes it (hipMemsetAsync).
 */
#ifndef EBOS_HIP_H
#define EBOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EBOS_ABI_VERSION 2

typedef void* ebos_stream_t; /* hipStream_t */

typedef enum ebos_status {
  EBOS_OK = 0,
  EBOS_ERR_INVALID_ARG = -1, /* null pointer, negative size, unsupported enum value       */
  EBOS_ERR_LAUNCH = -2,      /* hipLaunchKernel / hipMemsetAsync reported an error          */
  EBOS_ERR_UNSUPPORTED = -3, /* valid request this build has no kernel for                  */
  EBOS_ERR_SCRATCH = -4      /* caller-provided scratch buffer too small                    */
} ebos_status;

/* reference-time modes, src/warp.py:245-259 */
typedef enum ebos_reftime_mode {
  EBOS_REF_FIRST = 0,    /* t_ref = min t                                     (:248-249) */
  EBOS_REF_LAST = 1,     /* t_ref = max t                                     (:252-253) */
  EBOS_REF_FRACTION = 2, /* t_ref = tmin + (tmax - tmin) * fraction  (float/middle/before/after/random, :245-247) */
  EBOS_REF_TIMEBASE = 3  /* the `tminmax` argument holds (t_ref, period) itself instead of (min t, max t):
                            explicit reference_time / time_period of warp_event_from_optical_flow and
                            warp_event_2dof_xy (:292-293, 344-349) */
} ebos_reftime_mode;

/* image accumulation methods, src/event_image_converter.py:351-367 */
typedef enum ebos_splat_mode {
  EBOS_SPLAT_BILINEAR = 0, /* bilinear_vote_*  (:503-620)                                  */
  EBOS_SPLAT_COUNT = 1,    /* count_event_*    (:407-501): +1 on every in-bounds neighbour */
  EBOS_SPLAT_POLARITY = 2  /* "polarity" (:355-363): image is [b,2,h,w]; channel 0 <- p > 0 */
} ebos_splat_mode;

/* Optional timing of the dominant kernel (the tile accumulate pass of ebos_iwe_dense_slab_f32): between
 * ebos_profile_start(max_records) and ebos_profile_stop() every launch of that kernel carries a HIP event pair
 * stamped with the dispatch's own begin / end (hipExtLaunchKernelGGL) on the stream it runs on.  ebos_profile_stop synchronises those events, writes up to
 * `cap` durations in milliseconds to the HOST array `ms` and returns how many it wrote.  Not thread-safe;
 * off by default. */
int ebos_profile_start(int max_records);
int ebos_profile_stop(float* ms, int cap);
/* The same for another kernel of the path (one selector active at a time): */
typedef enum ebos_profile_kernel {
  EBOS_PROFILE_SLAB_ACCUMULATE = 0, /* iwe_slab_accumulate_kernel (what ebos_profile_start selects)                    */
  EBOS_PROFILE_TILED_BWD = 1,       /* iwe_dense_tiled_bwd_kernel of ebos_iwe_{dense,2dof,patch}_tiled_bwd_f32          */
  EBOS_PROFILE_SLAB_COMBINE = 2,    /* the slab combine pass (IWE assembly + variance) of ebos_iwe_*_slab_f32           */
  EBOS_PROFILE_GRADMAG_FUSED = 3    /* the Sobel pass of ebos_gradient_magnitude_fused_f32 (value partials + gradient)  */
} ebos_profile_kernel;
int ebos_profile_start_kernel(int which, int max_records);

int ebos_version(void);               /* EBOS_ABI_VERSION of the loaded library */
const char* ebos_last_error(void);    /* host string                            */
const char* ebos_build_info(void);    /* host string: arch, compiler, options   */

/* ------------------------------------------------------------------------------------------
 * A2  time range of an event batch.  Replaces nt_min/nt_max over events[..., 2]
 *     (src/warp.py:245-253, 283-287; src/types/__init__.py:21-47).
 *     events [b, n, 4] AoS; out tminmax [b, 2] = (min t, max t) per batch row.
 * ---------------------------------------------------------------------------------------- */
int ebos_time_range_f32(const float* events, int64_t b, int64_t n, float* tminmax, ebos_stream_t stream);
int ebos_time_range_f64(const double* events, int64_t b, int64_t n, double* tminmax, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A3  Warp.warp_event(..., "dense-flow")  (src/warp.py:193-228 -> :292-342, torch branch :330-342).
 *     dt = t - t_ref; if normalize_t: dt /= (max dt - min dt)            (:283-287)
 *     i  = trunc(x) * row_stride + trunc(y)                              (:334)
 *     x' = x - dt * flow[0][i];  y' = y - dt * flow[1][i];  t' = dt;  p' = p   (:335-337)
 *     Arithmetic is done in the element type with the reference's operation order and without
 *     FMA contraction, so the result is bit-identical to the reference on the same dtype.
 *     events/warped [b, n, 4]; flow [b, 2, H, W]; tminmax [b, 2] from ebos_time_range_*.
 *     row_stride = Warp.image_size[1].  An event whose source index falls outside [0, H*W)
 *     (torch.gather would raise) passes through un-displaced and increments *oob_count
 *     (device int32, nullable).
 * ---------------------------------------------------------------------------------------- */
int ebos_warp_dense_f32(const float* events, const float* flow, const float* tminmax, int ref_mode,
                        double ref_fraction, int normalize_t, int64_t b, int64_t n, int H, int W,
                        int row_stride, float* warped, int32_t* oob_count, ebos_stream_t stream);
int ebos_warp_dense_f64(const double* events, const double* flow, const double* tminmax, int ref_mode,
                        double ref_fraction, int normalize_t, int64_t b, int64_t n, int H, int W,
                        int row_stride, double* warped, int32_t* oob_count, ebos_stream_t stream);

/* autograd of A3 w.r.t. the flow: d_flow[c][i] += -dt * d_warped[..., c]
 * (accumulates; d_flow [b, 2, H, W]; d_warped [b, n, 4], columns 2,3 ignored). */
int ebos_warp_dense_bwd_f32(const float* events, const float* tminmax, int ref_mode, double ref_fraction,
                            int normalize_t, const float* d_warped, int64_t b, int64_t n, int H, int W,
                            int row_stride, float* d_flow, ebos_stream_t stream);
int ebos_warp_dense_bwd_f64(const double* events, const double* tminmax, int ref_mode, double ref_fraction,
                            int normalize_t, const double* d_warped, int64_t b, int64_t n, int H, int W,
                            int row_stride, double* d_flow, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A4  Warp.warp_event(..., "2d-translation" | "rigid-optical-flow")  (src/warp.py:344-383).
 *     x' = x + dt * theta[0]; y' = y + dt * theta[1]  (note the + sign, :368-375).  Un-batched.
 *     theta: device [2].  time_period: device [1] or NULL (then max dt - min dt, :285-286).
 *     bwd: d_theta[c] += sum_n dt * d_warped[n][c]  (accumulates, device [2]).
 * ---------------------------------------------------------------------------------------- */
int ebos_warp_2dof_f32(const float* events, const float* theta, const float* tminmax, int ref_mode,
                       double ref_fraction, int normalize_t, const float* time_period, int64_t n,
                       float* warped, ebos_stream_t stream);
int ebos_warp_2dof_f64(const double* events, const double* theta, const double* tminmax, int ref_mode,
                       double ref_fraction, int normalize_t, const double* time_period, int64_t n,
                       double* warped, ebos_stream_t stream);
int ebos_warp_2dof_bwd_f32(const float* events, const float* tminmax, int ref_mode, double ref_fraction,
                           int normalize_t, const float* time_period, const float* d_warped, int64_t n,
                           float* d_theta, ebos_stream_t stream);
int ebos_warp_2dof_bwd_f64(const double* events, const double* tminmax, int ref_mode, double ref_fraction,
                           int normalize_t, const double* time_period, const double* d_warped, int64_t n,
                           double* d_theta, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A7/A8/A10  EventImageConverter.bilinear_vote_tensor/_numpy, count_event_*, "polarity"
 *     (src/event_image_converter.py:407-620, 355-363).
 *     r0 = floor(x + eps), c0 = floor(y + eps); fr = x - r0, fc = y - c0;  R = r0 + pad_h, C = c0 + pad_w
 *     (R,C) += (1-fr)(1-fc) w; (R+1,C) += fr (1-fc) w; (R,C+1) += (1-fr) fc w; (R+1,C+1) += fr fc w
 *     each only when inside the [h, w] image (h, w = PADDED size, :34).  eps = 1e-6 for tensors
 *     (:586), 1e-8 for numpy arrays (:528).  Out-of-image taps are skipped (the reference adds 0
 *     to pixel 0, :617-618: identical for finite inputs).
 *     events [b, n, 4]; weight: device [b, n] or NULL (then weight_scalar, :576-577,611-614);
 *     image [b, h, w] ([b, 2, h, w] for EBOS_SPLAT_POLARITY).  Accumulates.
 * ---------------------------------------------------------------------------------------- */
int ebos_splat_f32(const float* events, const float* weight, double weight_scalar, int mode, double eps,
                   int64_t b, int64_t n, int h, int w, int pad_h, int pad_w, float* image,
                   ebos_stream_t stream);
int ebos_splat_f64(const double* events, const double* weight, double weight_scalar, int mode, double eps,
                   int64_t b, int64_t n, int h, int w, int pad_h, int pad_w, double* image,
                   ebos_stream_t stream);

/* autograd of the bilinear splat, G = d_image [b, h, w]:
 *   d_events[..., 0] = w [(1-fc)(G[R+1,C]-G[R,C]) + fc (G[R+1,C+1]-G[R,C+1])]
 *   d_events[..., 1] = w [(1-fr)(G[R,C+1]-G[R,C]) + fr (G[R+1,C+1]-G[R+1,C])]   (columns 2,3 = 0)
 *   d_weight[n]      = sum_taps tap_weight * G[tap]
 * d_events [b, n, 4] and d_weight [b, n] are overwritten; either may be NULL. */
int ebos_splat_bwd_f32(const float* events, const float* weight, double weight_scalar, double eps,
                       const float* d_image, int64_t b, int64_t n, int h, int w, int pad_h, int pad_w,
                       float* d_events, float* d_weight, ebos_stream_t stream);
int ebos_splat_bwd_f64(const double* events, const double* weight, double weight_scalar, double eps,
                       const double* d_image, int64_t b, int64_t n, int h, int w, int pad_h, int pad_w,
                       double* d_events, double* d_weight, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The ordered route of the same accumulation (csrc/splat_ordered.hip): a sorted index of the events by destination
 * cell, then one owner per pixel that sums its addends in a fixed order and writes the pixel with a plain store.  No
 * atomics on the image and no float atomics anywhere: the image is a pure function of the inputs, bit for bit -- call
 * after call, and for a batch row alone or inside any batch.  events, weight, mode, eps, sizes and padding mean what they
 * mean for ebos_splat_*; every tap is computed exactly as there.  ebos_splat_* stays the default route.
 *
 * Index.  Event i = row * n + e.  Its top-left tap (R, C) lies in the extended grid R in [-1, h-1], C in [-1, w-1], or
 * the event is dropped (none of its four taps is inside the image, or a coordinate is NaN, +-Inf or beyond 2^30).
 *     key = ((row * planes + plane) * (h + 1) + R + 1) * (w + 1) + C + 1        keys = b * planes * (h + 1) * (w + 1)
 * with planes = 2, plane = (p > 0 ? 0 : 1) for EBOS_SPLAT_POLARITY and planes = 1, plane = 0 otherwise.  The workspace
 * (ebos_splat_index_bytes bytes; 0 for sizes that are refused) starts with
 *     int32 offsets[keys + 1]     at byte 0
 *     int32 indices[b * n]        at the next multiple of 256 bytes
 * indices[offsets[k] .. offsets[k+1]) are the events of key k, ascending; the dropped events stand behind
 * offsets[keys].  The rest of the workspace is scratch of the build (a stable radix sort; the grouping does not depend on
 * the order in which anything executes).  An index serves any number of ebos_splat_ordered_* calls on the same events,
 * mode, eps, sizes and padding, with any weights.  b <= 65535; b * n and keys must stay below 2^31 (EBOS_ERR_INVALID_ARG).
 *
 * Summation order.  The addend list of pixel (row, plane, r, c) is the events of the cells (r-1, c-1), (r-1, c),
 * (r, c-1), (r, c) in this order, each cell in ascending event index; an event's addend is its tap on (r, c),
 *     fr fc wv,   fr (1-fc) wv,   (1-fr) fc wv,   (1-fr)(1-fc) wv          for the four cells,
 * evaluated in the element type as (x * y) * wv, every operation rounded on its own; wv = weight[i] or weight_scalar;
 * EBOS_SPLAT_COUNT adds 1 per addend.
 *   - a list of at most 256 addends:  s = +0, then s = s + addend in list order;
 *   - a longer list:  p[l] = +0, then p[l] = p[l] + addend[j] for j = l, l + 64, l + 128, ... ascending, l = 0 .. 63;
 *     then for off = 32, 16, 8, 4, 2, 1:  p[l] = p[l] + p[l + off] for l < off;  s = p[0].
 * Every pixel of image [b, h, w] ([b, 2, h, w] for polarity) is overwritten (+0 without addends): the caller need not
 * zero it.  The backward of this route is ebos_splat_bwd_*.
 * ---------------------------------------------------------------------------------------- */
size_t ebos_splat_index_bytes(int64_t b, int64_t n, int h, int w, int mode);
int ebos_splat_index_build_f32(const float* events, int mode, double eps, int64_t b, int64_t n, int h, int w,
                               int pad_h, int pad_w, void* index, size_t index_bytes, ebos_stream_t stream);
int ebos_splat_index_build_f64(const double* events, int mode, double eps, int64_t b, int64_t n, int h, int w,
                               int pad_h, int pad_w, void* index, size_t index_bytes, ebos_stream_t stream);
int ebos_splat_ordered_f32(const float* events, const float* weight, double weight_scalar, int mode, double eps,
                           int64_t b, int64_t n, int h, int w, int pad_h, int pad_w, const void* index,
                           size_t index_bytes, float* image, ebos_stream_t stream);
int ebos_splat_ordered_f64(const double* events, const double* weight, double weight_scalar, int mode, double eps,
                           int64_t b, int64_t n, int h, int w, int pad_h, int pad_w, const void* index,
                           size_t index_bytes, double* image, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Event plan: the device-resident, iteration-invariant form of one event window used by the
 * fused hot path.  (x, y, t, p) of every event are constant across solver iterations and flow
 * hypotheses: only the motion changes, so this is built once per window.
 *
 * ebos_events_to_soa_*: AoS [n,4] -> SoA f32 (x, y, dt, p).  dt follows src/warp.py:264-288
 * but is evaluated in fp64 and rounded once to f32 (absolute timestamps of ~10 s do not
 * survive f32).
 * ---------------------------------------------------------------------------------------- */
int ebos_events_to_soa_f32(const float* events, const float* tminmax, int ref_mode, double ref_fraction,
                           int normalize_t, int64_t n, float* x, float* y, float* dt, float* p,
                           ebos_stream_t stream);
int ebos_events_to_soa_f64(const double* events, const double* tminmax, int ref_mode, double ref_fraction,
                           int normalize_t, int64_t n, float* x, float* y, float* dt, float* p,
                           ebos_stream_t stream);

/* Raw sensor columns -> SoA (event ingest).  The CCS recordings hold
 * raw_events/{x: int16 column, y: int16 row, t: int32 microseconds, p: bool}
 * (src/data_loader/ccs.py:57-66); the reference expands a window on the host to float64 [n, 4] =
 * (y, x, t / 1e6, p) (src/data_loader/ccs.py:289-297) before Warp sees it.  These two entry points
 * take the 9 B/event raw window as it is on the device and produce the same SoA plan as
 * ebos_events_to_soa_f64 on that float64 array (bit-identical: the same fp64 time arithmetic).
 *   t_bytes: 4 (int32) or 8 (int64) ticks; ticks_per_second: 1e6 for microseconds.
 *   ebos_raw_time_range: tminmax[2] (device, seconds) = (min t, max t) / ticks_per_second;
 *     scratch_ticks: device int64[2].  n >= 1.
 *   ebos_raw_events_to_soa: ref_mode / ref_fraction / normalize_t as ebos_events_to_soa_*. */
int ebos_raw_time_range(const void* t, int t_bytes, int64_t n, double ticks_per_second, int64_t* scratch_ticks,
                        double* tminmax, ebos_stream_t stream);
int ebos_raw_events_to_soa(const int16_t* col, const int16_t* row, const void* t, int t_bytes,
                           const uint8_t* pol, double ticks_per_second, const double* tminmax, int ref_mode,
                           double ref_fraction, int normalize_t, int64_t n, float* x, float* y, float* dt,
                           float* p, ebos_stream_t stream);

/* Source-tile binning (counting sort by source pixel, tile-major).  The image [H, W] is cut into
 * tiles of tile_h x tile_w pixels; key(event) = tile_id * tile_h*tile_w + pixel-in-tile of
 * (trunc(x), trunc(y)).  Events are reordered by key; events of one tile, and of one source
 * pixel, become contiguous (coalesced flow reads forward, segmented reduction backward).
 *   n_keys = tiles_y * tiles_x * tile_h * tile_w,  tiles_y = ceil(H / tile_h), tiles_x = ceil(W / tile_w)
 *   key_offsets [n_keys + 1] (int32, out): exclusive prefix sum of the per-key counts;
 *       tile t owns sorted positions [key_offsets[t * tile_h*tile_w], key_offsets[(t+1) * tile_h*tile_w])
 *   perm [n] (int32, out): original index of the event at each sorted position
 *   scratch: >= ebos_bin_scratch_bytes(n_keys) bytes
 *   oob_count (device int32, nullable): events whose source pixel is outside the image; they are
 *       dropped from the plan (torch.gather would raise for them, src/warp.py:334-336).
 *   frac_count (device int32, nullable): number of kept events with a fractional / negative source
 *       coordinate; the compact plan (ebos_plan_compact_f32) is valid iff it stays 0.
 * All SoA outputs must be 16-byte aligned and padded to a multiple of 4 elements (vector loads).
 * The order of events inside one source pixel is not deterministic (atomic cursor). */
size_t ebos_bin_scratch_bytes(int64_t n_keys);
/* scratch size that lets ebos_bin_events_f32 scatter one aligned 32-byte record per event (then unpacked to the SoA
 * arrays by a streaming pass) instead of five 4-byte stores to five arrays; with only ebos_bin_scratch_bytes(n_keys)
 * the five-store form runs.  Never smaller than ebos_bin_scratch_bytes(n_keys). */
size_t ebos_bin_scratch_bytes_events(int64_t n, int H, int W, int tile_h, int tile_w);
int ebos_bin_events_f32(const float* x, const float* y, const float* dt, const float* p, int64_t n,
                        int H, int W, int tile_h, int tile_w, float* xs, float* ys, float* dts, float* ps,
                        int32_t* perm, int32_t* key_offsets, int32_t* oob_count, int32_t* frac_count,
                        void* scratch, size_t scratch_bytes, ebos_stream_t stream);

/* Adaptive work items for the tile-private forward kernels.  With one workgroup per tile the pass lasts as long as
 * the fullest tile; real windows are far from uniform (a schlieren object in front of a static background).
 * ebos_plan_parts cuts heavy tiles into parts: parts(t) = max(1, ceil(load(t) / tau)), where tau balances the
 * longest work item against the average load of a CU:  tau + F = (N + items(tau) F) / n_cu  (n_cu = CUs of the
 * device, F = fixed_events = the per-item fixed work in events: 8192 for a 10 M-event window or few tiles on many CUs;
 * where the tiles fill the device an extra item is an extra round and ~6.5e10 / N was measured best -- 32 k at 2 M events,
 * at most 65536: EventPlan's part_fixed_events), within a budget of 2 x tiles work
 * items.  A uniform window keeps one part per tile.  part_table (int32, out, 5 tiles + 1 entries):
 *     [0, tiles]               part_off: first slab of each tile (part_off[tiles] = work items in use)
 *     [tiles + 1, 3 tiles]     item_tile: tile of each of the 2 x tiles work items, heaviest first (the dispatcher
 *                              then schedules longest-processing-time first), -1 = unused
 *     [3 tiles + 1, 5 tiles]   item_part: which part of that tile
 * Pass it with splits = 0 to ebos_iwe_dense_slab_f32 / ebos_iwe_2dof_slab_f32 (workspace sized with splits = 0). */
int ebos_plan_parts(const int32_t* key_offsets, int H, int W, int tile_h, int tile_w, int n_cu, int fixed_events,
                    int32_t* part_table, ebos_stream_t stream);

/* What the host wants to know about a freshly built plan, as four int32 side by side (one small launch, one 16-byte copy):
 *     facts[0] = counts[0]   events outside the image (dropped)      facts[2] = part_table[tiles]  work items in use
 *     facts[1] = counts[1]   events with fractional source pixels    facts[3] = events of the fullest source tile
 * counts = {oob_count, frac_count} of ebos_bin_events_f32 / the counts pair of ebos_plan_lean (NULL: 0), part_table of
 * ebos_plan_parts (NULL: 0).  The reference has no counterpart: its loader crops on the host (src/solver/patch_eklt.py:262-281);
 * the fullest tile decides between the resident solver kernel and the four launches (solver/fused_loop.py: crowded_for_resident). */
int ebos_plan_facts(const int32_t* key_offsets, int H, int W, int tile_h, int tile_w, const int32_t* counts,
                    const int32_t* part_table, int32_t* facts, ebos_stream_t stream);

/* Lean plan build: the compact plan (below) straight from the window -- AoS float32 / float64 [n, 4] = (x = row, y = col, t, p)
 * as the reference's loader hands it over (src/data_loader/ccs.py:289-297), or the raw sensor columns (:57-66) -- without
 * the SoA arrays and the permutation that only per-event weights and fractional source coordinates need.  The window is read
 * ONCE: every chunk of it is counting-sorted by (tile, row band) inside LDS and staged as a coalesced stream, one workgroup per
 * band then gathers its runs, sorts them by source pixel in LDS and puts every pixel's events in ascending dt (two builds of one
 * window hold identical arrays, whatever the length of a pixel's run); no global atomics per event, no scattered writes.  Outputs exactly what ebos_bin_events_f32 +
 * ebos_plan_compact_f32 produce:
 *     key_offsets [n_keys + 1], grp_offsets [tiles + 1], cpix / cdt [capacity_slots >= n + 3 tiles + 4]
 * (the order of the events inside one source pixel is unspecified in both), plus
 *     counts [2] (device int32): events outside the image (dropped), kept events with a fractional / negative source
 *                coordinate -- the plan is valid iff counts[1] == 0;
 *     tminmax [2] (device double, nullable): (min t, max t) of the window in seconds.
 *   source: 0 = `events` float32 [n, 4], 1 = `events` float64 [n, 4], 2 / 3 = raw columns with int32 / int64 ticks.
 *   ref_mode: EBOS_REF_FIRST / LAST / FRACTION; dt = (t - t_ref) [/ (tmax - tmin) if normalize_t], evaluated in fp64.
 *   scratch: >= ebos_plan_lean_scratch_bytes(...) bytes (10 B per event + the chunks' bin tables).  1 <= n < 2^31. */
size_t ebos_plan_lean_scratch_bytes(int64_t n, int H, int W, int tile_h, int tile_w);
int ebos_plan_lean(int source, const void* events, const int16_t* col, const int16_t* row, const void* t,
                   double ticks_per_second, int64_t n, int ref_mode, double ref_fraction, int normalize_t, int H, int W,
                   int tile_h, int tile_w, int32_t* key_offsets, int32_t* grp_offsets, uint16_t* cpix, float* cdt,
                   int64_t capacity_slots, int32_t* counts, double* tminmax, void* scratch, size_t scratch_bytes,
                   ebos_stream_t stream);
/* The lean plans of SEVERAL windows of one recording in one set of launches.  col / row / t (int32, or int64 with t_is_64): the
 * device columns of n_total raw events; ranges: HOST int64 [n_windows, 2], window w = events [begin, end) of the columns -- ranges
 * may overlap, be empty and come in any order.  Every window is built exactly as ebos_plan_lean builds events [begin, end) on their
 * own -- its own reference time and normalisation, the same bits in every output -- into shared buffers:
 *     key_offsets + w * key_stride  [n_keys + 1]      grp_offsets + w * grp_stride  [tiles + 1]      counts + 2 w      tminmax + 2 w
 *     cpix / cdt + slot_offsets[w]: slot_offsets HOST int64 [n_windows + 1], ascending, each a multiple of 8 (16-byte aligned
 *         slots), slot_offsets[w + 1] - slot_offsets[w] >= n_w + 3 tiles + 4.
 * An empty window leaves key_offsets and grp_offsets zero, counts zero and tminmax undefined.  The stage, totals and bin-sort passes
 * run once for every 64 windows (the windows' descriptors travel in the kernel arguments); the staging pass's grid is the windows'
 * chunks one after the other, so no window is padded to the largest.  The host-only size query takes the same ranges: the sum of
 * ebos_plan_lean_scratch_bytes over the windows.  Returns EBOS_ERR_UNSUPPORTED -- before anything is launched -- when ANY window's
 * geometry is outside the LDS sort (as ebos_plan_lean would for it): build the windows one by one then. */
size_t ebos_plan_lean_batch_scratch_bytes(const int64_t* ranges, int n_windows, int H, int W, int tile_h, int tile_w);
int ebos_plan_lean_batch(const int16_t* col, const int16_t* row, const void* t, int t_is_64, double ticks_per_second, int64_t n_total,
                         const int64_t* ranges, int n_windows, int ref_mode, double ref_fraction, int normalize_t, int H, int W,
                         int tile_h, int tile_w, int32_t* key_offsets, int64_t key_stride, int32_t* grp_offsets, int64_t grp_stride,
                         uint16_t* cpix, float* cdt, const int64_t* slot_offsets, int32_t* counts, double* tminmax, void* scratch,
                         size_t scratch_bytes, ebos_stream_t stream);
/* ebos_plan_parts / ebos_plan_facts for n_windows plans of one geometry laid out as above, one launch each (a workgroup per plan;
 * parts: one launch per 64 plans): part_table + w * part_stride [5 tiles + 1]; fixed_events: HOST int32 [n_windows], the per-item
 * fixed work of each window; counts [n_windows, 2] (nullable), facts [n_windows, 4] (device; one copy reads them all back). */
int ebos_plan_parts_batch(const int32_t* key_offsets, int64_t key_stride, int n_windows, int H, int W, int tile_h, int tile_w, int n_cu,
                          const int32_t* fixed_events, int32_t* part_table, int64_t part_stride, ebos_stream_t stream);
int ebos_plan_facts_batch(const int32_t* key_offsets, int64_t key_stride, int n_windows, int H, int W, int tile_h, int tile_w,
                          const int32_t* counts, const int32_t* part_table, int64_t part_stride, int32_t* facts, ebos_stream_t stream);
/* Compact plan: the 6 B/event layout of the tile-private kernels, valid when every source coordinate is a
 * non-negative integer (frac_count == 0; camera events always are).  Per tile t the events occupy the groups
 * [grp_offsets[t], grp_offsets[t+1]) of 4 slots (16-byte vector loads, tiles start on a group boundary):
 *     cpix (u16) = (row_in_tile << 8) | col_in_tile          cdt (f32) = dt, NaN in padding slots
 * grp_offsets [tiles + 1] int32; cpix / cdt hold capacity_slots >= n + 3 tiles + 4 elements, 16-byte aligned.
 * Inputs are the binned arrays of ebos_bin_events_f32 (same tile size, tile_h, tile_w <= 256). */
int ebos_plan_compact_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                          int H, int W, int tile_h, int tile_w, int32_t* grp_offsets, uint16_t* cpix, float* cdt,
                          int64_t capacity_slots, ebos_stream_t stream);
/* The compact plan of a window whose source coordinates are FRACTIONAL (events rectified with a sub-pixel map or already warped by an earlier stage;
 * the flow is looked up at the truncated coordinate, src/warp.py:334): cpix / cdt as above from floor(x),
 * floor(y), plus cfx / cfy [capacity_slots] f32 = x - floor(x), y - floor(y) per slot (0 in padding slots).  Same information as
 * the (x, y, dt) arrays it is made from; read by the resident 2-DoF launch (ebos_cmax_2dof_problem::cfx / cfy). */
int ebos_plan_compact_frac_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                               int H, int W, int tile_h, int tile_w, int32_t* grp_offsets, uint16_t* cpix, float* cdt,
                               float* cfx, float* cfy, int64_t capacity_slots, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused hot path, dense flow: A3 + A7 in one pass, nothing materialised
 *   (src/warp.py:330-342 + src/event_image_converter.py:581-620), eps = 1e-6.
 *   x, y, dt, weight(nullable): SoA f32 [n];  flow [2, H, W];  iwe [h, w] with h = H + 2 pad_h ...
 *   Accumulates into iwe.
 * ebos_iwe_dense_f32        any event order; one global float atomic per tap.
 * ebos_iwe_dense_tiled_f32  binned events (ebos_bin_events_f32 with the same tile_h/tile_w):
 *   one workgroup per (tile, split) accumulates into an LDS image of the tile plus `halo` pixels
 *   on every side and flushes it once; taps beyond the halo fall back to global atomics, so the
 *   result is correct for any flow magnitude.  halo must be one of the built values
 *   (ebos_tiled_config lists them).  splits >= 1 workgroups share one tile's events.
 * ---------------------------------------------------------------------------------------- */
int ebos_iwe_dense_f32(const float* x, const float* y, const float* dt, const float* weight, int64_t n,
                       const float* flow, int H, int W, int row_stride, int pad_h, int pad_w, float* iwe,
                       ebos_stream_t stream);
int ebos_iwe_dense_tiled_f32(const float* xs, const float* ys, const float* dts, const float* weight,
                             const int32_t* key_offsets, int64_t n, const float* flow, int H, int W,
                             int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w,
                             float* iwe, ebos_stream_t stream);
/* number of supported (tile_h, tile_w, halo) triples; fills up to `cap` triples into out[3*i..] (host) */
int ebos_tiled_config(int* out, int cap);

/* backward of the fused dense path: G = a * g_image + c (g_image [h, w]; pass a = 1, c = 0 for a plain
 * upstream gradient; the variance cost folds its gradient 2 (IWE - mean)/(M-1) into (a, c) read from
 * the device array affine[2] so that no d_iwe image is materialised; affine may be NULL).
 *   d_flow[c][i] += -dt * dL/d(x',y')   with dL/dx', dL/dy' as in ebos_splat_bwd_*.
 * sorted != 0 promises that events sharing a source pixel are contiguous (binned plan): contributions
 * are pre-reduced across the wavefront with shuffles and one atomic per run is issued.
 * g_lo/g_hi: rows/cols [g_lo, h - g_lo) x [g_lo, w - g_lo) of g_image are valid, G = 0 elsewhere
 * (omit_boundary of the costs: g_lo = 1).  Accumulates into d_flow [2, H, W]. */
int ebos_iwe_dense_bwd_f32(const float* x, const float* y, const float* dt, const float* weight, int64_t n,
                           const float* flow, int H, int W, int row_stride, int pad_h, int pad_w,
                           const float* g_image, const float* affine, int g_lo, int sorted, float* d_flow,
                           float* d_weight, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Tile-private pipeline (the fast path): same mathematics as ebos_iwe_dense_tiled_f32 /
 * ebos_iwe_dense_bwd_f32, organised so that no global float atomic and no zero-fill is left.
 *
 * ebos_iwe_dense_slab_f32   forward.  Each (tile, split) workgroup accumulates its tile + halo in LDS
 *   (f64) and writes it once as a plain f32 "slab"; a combine pass sums the slabs covering each pixel,
 *   OVERWRITES iwe [h, w] (no caller-side zeroing) and, if want_variance, also reduces the variance of
 *   the image (omit_boundary as in the costs) into out_variance [1] (f32, nullable) and
 *   moments [2] = (mean, M) (f64, nullable) -- the contrast cost of SURVEY.md A14 at no extra pass.
 *   want_variance = 2: only the (sum, sum of squares) partials are left in the workspace (ebos_iwe_slab_partials),
 *   no finalize launch; out_variance / moments are not touched.
 *   workspace: >= ebos_iwe_slab_workspace_bytes(...) bytes, ZERO-FILLED ONCE by the caller when it is
 *   allocated; the kernels keep its spill section (taps beyond the halo) zero between calls, and a word behind the partials
 *   holds the number of the last call whose accumulate pass wrote spill taps (the combine pass reads the spill section only
 *   for that call).  One workspace serves one stream at a time.
 *   Results are deterministic (fixed summation order) except for taps beyond the halo.
 *   splits >= 1: every tile is cut into `splits` equal parts (workgroups); splits = 0: the adaptive work items of
 *   part_table (ebos_plan_parts; NULL otherwise).
 * ebos_iwe_dense_tiled_bwd_f32   backward.  One workgroup per tile: upstream image tile in LDS,
 *   wavefront-segmented sums per source pixel, d_flow [2, H, W] OVERWRITTEN with plain stores
 *   (binned plans only; g_image/affine/g_lo/d_weight as in ebos_iwe_dense_bwd_f32; d_weight in plan order).
 *   var_moments [2] (f64: mean, M of ebos_iwe_dense_slab_f32) + upstream [1] (f32), both nullable together: the
 *   loss is upstream * var(g_image) with g_image = the IWE itself; its gradient 2 (IWE - mean) / (M - 1) is folded
 *   into the kernel (no d_iwe image, no affine launch).
 *   addend [2, H, W] (nullable): added to the result as it is stored -- the gradient of the flow regularisers
 *   (ebos_flow_regularisers_f32), so that d_flow is the gradient of the whole objective without another pass.
 *   part_table (nullable): the adaptive work items of ebos_plan_parts -- every part of a tile writes a partial d_flow
 *   tile into the slab section of `workspace` (the forward workspace sized with splits = 0; its slabs are dead once
 *   the IWE is combined) and a second small kernel sums the parts.  workspace may be NULL when part_table is.
 * grp_offsets / cpix / cdt (nullable trio): the compact plan of ebos_plan_compact_f32; when given and weight is
 *   NULL, xs/ys/dts are not read (6 B/event instead of 12).  All SoA arrays are read 4 events (16 bytes) per
 *   lane: 16-byte aligned, padded to a multiple of 4 elements.
 * (tile_h, tile_w, halo) must be one of ebos_slab_config() -- or halo = EBOS_HALO_AUTO(max_halo, q):
 *
 * RUN-TIME WINDOWS.  Every `halo` argument / field of this section also takes EBOS_HALO_AUTO(max_halo, q) (a negative number):
 *   (tile_h, tile_w, max_halo) is a built configuration -- it sizes the LDS, the slabs and the workspace -- and every work item
 *   chooses ITS OWN window (hr rows, hc columns of halo per side, hc a multiple of 4, both <= max_halo) inside the kernel, from a
 *   bound on its displacements: max |flow| over the tile's own pixels (dense flow), over the grid cells its pixels interpolate
 *   (patch grid), or |theta| (2-DoF), times q / 64 >= max |dt| over the plan's events (1.0 -> q = 64 with normalised time and
 *   reference time inside the window; ebos_halo_auto rounds a bound up for you).  LDS clear / decode, slab traffic, the combine
 *   pass's reads and the backward kernel's upstream tile shrink with the window; BOS displacements are a few pixels, the +-30 px
 *   of the sampler range (configs/hot_plate1.yaml:46-80) is the search bound, not the operating point.  Taps beyond a window go to
 *   the spill image exactly as with a built halo, so the choice moves time, never results: images are bit-identical to those of
 *   the built max_halo as long as nothing spills.  Compact plans with unit weights (the lean loops); other calls run max_halo.
 *   The forward pass records each tile's window behind the SpillEpoch word of its workspace for its combine pass.
 * ---------------------------------------------------------------------------------------- */
#define EBOS_HALO_AUTO(max_halo, dt_bound_q64) (-((int)(max_halo) + 256 * (int)(dt_bound_q64)))
int ebos_halo_auto(int max_halo, double dt_bound); /* EBOS_HALO_AUTO(max_halo, ceil(64 dt_bound)); max_halo itself if out of range */
int ebos_slab_config(int* out, int cap);
size_t ebos_iwe_slab_workspace_bytes(int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h,
                                     int pad_w);
/* want_variance = 2 in ebos_iwe_dense_slab_f32 / ebos_iwe_2dof_slab_f32 leaves the variance as (sum, sum of squares)
 * partials in the workspace and skips the finalize launch; this (host-only) call tells where they are: byte offset
 * inside the workspace, number of partial pairs, and the pixel count M the variance refers to. */
int ebos_iwe_slab_partials(int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w,
                           int omit_boundary, size_t* offset_bytes, int64_t* n_partials, int64_t* n_pixels);
int ebos_iwe_dense_slab_f32(const float* xs, const float* ys, const float* dts, const float* weight,
                            const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt,
                            const int32_t* key_offsets, int64_t n, const float* flow, int H, int W, int tile_h,
                            int tile_w, int halo, int splits, int pad_h, int pad_w, void* workspace,
                            size_t workspace_bytes, float* iwe, int want_variance, int omit_boundary,
                            float* out_variance, double* moments, const int32_t* part_table,
                            ebos_stream_t stream);
/* One call for the objective AND its gradient -- the drop-in autograd path (plan.contrast_dense(flow).backward(), i.e.
 * warp.py:330-342 + event_image_converter.py:581-620 + torch.var and what autograd derives) costs what its kernels
 * cost only if the host does not marshal ~60 arguments through two calls per iteration.  ebos_dense_job holds everything
 * that is constant per (plan, padding, halo, splits): the caller fills it ONCE (plain pointers / sizes, same meaning as the
 * arguments of ebos_iwe_dense_slab_f32 / ebos_iwe_dense_tiled_bwd_f32) and passes its address afterwards.
 *   iwe [h, w] and moments [2] are scratch outputs owned by the job (IWE and (mean, M) of the LAST evaluation).
 * ebos_variance_dense_job_f32: out_variance[0] = var(IWE(flow)) (omit_boundary as in the costs); if d_flow != NULL also
 *   d_flow [2, H, W] = upstream[0] * d var / d flow (upstream: device f32 [1]; NULL = 1).  Enqueues accumulate, combine and
 *   finalize on `stream` -- or, with d_flow, accumulate, combine and the tile-private backward, which reduces the variance
 *   partials of the combine pass itself and writes out_variance / moments (three launches, no finalize); no host
 *   synchronisation. */
typedef struct ebos_dense_job {
  const float *xs, *ys, *dts;          /* (x, y, dt) plan, nullable when the compact trio is given */
  const int32_t* grp_offsets;          /* compact plan (ebos_plan_compact_f32), nullable trio      */
  const uint16_t* cpix;
  const float* cdt;
  const int32_t* key_offsets;
  int64_t n;
  int H, W, tile_h, tile_w, halo, splits, pad_h, pad_w, omit_boundary;
  void* workspace;                     /* >= ebos_iwe_slab_workspace_bytes(...), zero-filled once   */
  size_t workspace_bytes;
  const int32_t* part_table;           /* adaptive work items (splits == 0), else nullable          */
  float* iwe;                          /* [H + 2 pad_h, W + 2 pad_w]                                */
  double* moments;                     /* [2]                                                       */
} ebos_dense_job;
int ebos_variance_dense_job_f32(const ebos_dense_job* job, const float* flow, float* out_variance, const float* upstream,
                                float* d_flow, ebos_stream_t stream);
/* The same for the gradient-magnitude contrast (BASELINE configs[2]; SURVEY.md A14: mean squared Sobel gradient of the IWE,
 * src/utils/stat_utils.py:69-92, 117-139): out_contrast[0] = gradient_magnitude(IWE(flow)); with d_flow != NULL also
 * d_flow [2, H, W] = upstream[0] * d contrast / d flow.  Enqueues accumulate, combine, ONE Sobel pass (value partials + gradient
 * image, ebos_gradient_magnitude_fused_f32) and the tile-private backward, whose first workgroup sums the value partials: four
 * launches, no finalize, no host synchronisation.  d_iwe [h, w] f32 and partials [ebos_gradient_magnitude_fused_partials(h, w)]
 * f64 are scratch of the caller's (job->moments is not used).  out_scaled (nullable): see ebos_variance_dense_job_signed_f32. */
int ebos_gradient_magnitude_dense_job_f32(const ebos_dense_job* job, const float* flow, float* out_contrast, float* out_scaled,
                                          const float* upstream, float* d_flow, float* d_iwe, double* partials, int64_t n_partials,
                                          ebos_stream_t stream);
/* ebos_variance_dense_job_f32 with one more output for a cost that has a DIRECTION (the cost plugins of src/costs: "minimize" negates the contrast):
 * out_scaled[0] = upstream[0] * variance (nullable; needs d_flow), written by the backward kernel's first workgroup beside
 * out_variance -- the signed loss and its gradient come out of the three launches, no kernel negates a scalar or scales 7.4 MB.
 * (ebos_gradient_magnitude_dense_job_f32 takes the same out_scaled.) */
int ebos_variance_dense_job_signed_f32(const ebos_dense_job* job, const float* flow, float* out_variance, float* out_scaled,
                                       const float* upstream, float* d_flow, ebos_stream_t stream);
int ebos_iwe_dense_tiled_bwd_f32(const float* xs, const float* ys, const float* dts, const float* weight,
                                 const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt,
                                 const int32_t* key_offsets, int64_t n, const float* flow, int H, int W,
                                 int tile_h, int tile_w, int halo, int pad_h, int pad_w, const float* g_image,
                                 const float* affine, int g_lo, float* d_flow, float* d_weight,
                                 const double* var_moments, const float* upstream, const float* addend,
                                 void* workspace, size_t workspace_bytes, const int32_t* part_table,
                                 ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same pipeline with the flow given as a PATCH GRID [2, gh, gw] (the parameters of the patch solvers,
 * src/solver/patch_eklt.py:173-204: dense = crop(resize(replicate_pad(grid)))): every workgroup evaluates the
 * grid -> dense map for its own source tile into LDS and the event loop takes the flow from there -- no dense
 * [2, H, W] field, no upsample launch, LDS reads instead of L2 gathers ("fused into the warp's flow
 * fetch").  Same results as ebos_upsample_patch_flow_f32 + ebos_iwe_dense_slab_f32 (one shared expression).
 *
 * ebos_patch_fused_supported   1 when (tile, halo) leaves LDS for the tile's flow and a tile + 2 px apron touches at most
 *   16 x 16 grid cells ((tile + 4) / slide + 3 <= 16 per axis); 0 otherwise (use the upsample + dense entry points).
 * ebos_iwe_patch_slab_f32      forward; arguments as ebos_iwe_dense_slab_f32 with (grid, gh, gw, patch, slide) in place
 *   of flow; compact plans with unit weights only.
 * ebos_iwe_patch_tiled_bwd_f32 backward; instead of d_flow every work item writes the adjoint of the grid -> dense map
 *   restricted to its tile: <= 16 x 16 partial cell gradients per flow component into grad_partials
 *   (ebos_patch_grad_partials_bytes; adaptive = part_table != NULL).  addend [2, H, W] (nullable) enters once per tile.
 *   w_flow_norm / w_image_gradient != 0: the flow regularisers w * mean |flow| (src/costs/flow_norm.py:45-56, pointwise) and
 *   w * mean(|d flow / d row| + |d flow / d col|) (src/costs/image_gradient.py:60-75, torch.gradient lines, unit weights) are
 *   evaluated on the flow the tile holds in LDS (with a 2 px apron): gradient added here, value as one f64 partial per work item in
 *   reg_partials [ebos_patch_grad_partials_bytes / 2048] (slots of unused work items are not written: zero the buffer
 *   once) -- no dense field and no ebos_flow_regularisers_f32 launch.
 *   var_partials (nullable; then var_moments must be NULL and upstream given): the (sum, sum of squares) partials that the
 *   forward call left with want_variance = 2 (ebos_iwe_slab_partials tells where).  Every workgroup reduces them itself
 *   (14 KB of L2 reads) and folds the variance gradient in; workgroup 0 also writes out_variance [1] / out_moments [2]
 *   (nullable) -- the finalize launch between forward and backward disappears.
 * ebos_patch_grad_combine_adam_f32   d_grid [2, gh, gw] := sum of the partials of the tiles touching each cell, times
 *   grad_mask (nullable); with theta != NULL also the Adam step and loss bookkeeping of
 *   ebos_upsample_patch_flow_bwd_adam_f32 (same arguments).  theta == NULL: plain gradient (optimiser arguments unused).
 * Together they replace upsample -> dense slab -> dense tiled bwd -> adjoint rows -> adjoint cols (+ Adam): five
 * launches become three and the [2, H, W] flow / gradient fields disappear.
 * ---------------------------------------------------------------------------------------- */
int ebos_patch_fused_supported(int tile_h, int tile_w, int halo, int slide_h, int slide_w);
/* ebos_iwe_slab_batch_f32  n_windows INDEPENDENT windows of one geometry (the time windows of bos_event.py:144-220, BASELINE
 *   configs[3]) per call: accumulate, combine and finalize each run as ONE launch over (work item, window) for up to 16 windows
 *   at a time -- thin windows are bound by per-launch fixed work, and at one workgroup per CU consecutive accumulate launches
 *   cannot overlap.  Per window: its compact plan (unit weights), its flow -- a dense field [2, H, W] when gh == gw == 0, else
 *   a patch grid [2, gh, gw] (arguments as ebos_iwe_patch_slab_f32) --, its OWN workspace (each >= workspace_bytes >=
 *   ebos_iwe_slab_workspace_bytes, zero-filled once), iwe [h, w] and variance outputs.  Needs w and pad_w multiples of 4.
 *   Results are bit-identical to n_windows calls of ebos_iwe_dense_slab_f32 / ebos_iwe_patch_slab_f32.  `windows` is a HOST
 *   array, read before the call returns.  tail_stream (nullable): a second stream of the caller's for the combine / finalize
 *   passes, which need no LDS and then run beside the accumulate pass of the next 16 windows; `stream` is made to wait for it
 *   before the call returns, so the results are ordered on `stream` either way. */
typedef struct ebos_slab_window {
  const int32_t* grp_offsets;  /* the window's compact plan (ebos_plan_lean / ebos_plan_events_*)                 */
  const uint16_t* cpix;
  const float* cdt;
  const int32_t* key_offsets;
  const int32_t* part_table;   /* adaptive work items (splits == 0), else nullable                               */
  const float* flow;           /* [2, H, W], or the patch grid [2, gh, gw]                                        */
  void* workspace;             /* this window's own, zero-filled once                                             */
  float* iwe;                  /* [H + 2 pad_h, W + 2 pad_w], overwritten                                         */
  float* out_variance;         /* [1], nullable                                                                   */
  double* moments;             /* [2] (mean, M), nullable                                                         */
} ebos_slab_window;
int ebos_iwe_slab_batch_f32(const ebos_slab_window* windows, int n_windows, int gh, int gw, int patch_h, int patch_w, int slide_h,
                            int slide_w, int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w,
                            size_t workspace_bytes, int want_variance, int omit_boundary, ebos_stream_t stream,
                            ebos_stream_t tail_stream);

int ebos_iwe_patch_slab_f32(const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt,
                            const int32_t* key_offsets, int64_t n, const float* grid, int gh, int gw, int patch_h,
                            int patch_w, int slide_h, int slide_w, int H, int W, int tile_h, int tile_w, int halo,
                            int splits, int pad_h, int pad_w, void* workspace, size_t workspace_bytes, float* iwe,
                            int want_variance, int omit_boundary, float* out_variance, double* moments,
                            const int32_t* part_table, ebos_stream_t stream);
/* ... on a window of FRACTIONAL source coordinates (undistorted events): the arrays of ebos_plan_compact_frac_f32 -- the compact slots
 * with x - floor(x), y - floor(y) per slot.  The general event loop on the compact layout (cfx == cfy == NULL: ebos_iwe_patch_slab_f32). */
int ebos_iwe_patch_slab_frac_f32(const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt, const float* cfx, const float* cfy,
                                 const int32_t* key_offsets, int64_t n, const float* grid, int gh, int gw, int patch_h, int patch_w,
                                 int slide_h, int slide_w, int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h,
                                 int pad_w, void* workspace, size_t workspace_bytes, float* iwe, int want_variance, int omit_boundary,
                                 float* out_variance, double* moments, const int32_t* part_table, ebos_stream_t stream);
size_t ebos_patch_grad_partials_bytes(int H, int W, int tile_h, int tile_w, int adaptive);
int ebos_iwe_patch_tiled_bwd_f32(const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt,
                                 const int32_t* key_offsets, int64_t n, const float* grid, int gh, int gw,
                                 int patch_h, int patch_w, int slide_h, int slide_w, int H, int W, int tile_h,
                                 int tile_w, int halo, int pad_h, int pad_w, const float* g_image,
                                 const float* affine, int g_lo, const double* var_moments, const float* upstream,
                                 const float* addend, float* grad_partials, size_t grad_partials_bytes,
                                 const int32_t* part_table, float w_flow_norm, float w_image_gradient,
                                 double* reg_partials,
                                 const double* var_partials, int64_t n_var_partials, int64_t n_var_pixels,
                                 float* out_variance, double* out_moments, ebos_stream_t stream);
/* The same backward for the contrast of the 3-tap BLURRED image (iwe.blur_sigma > 0, src/event_image_converter.py:399-404):
 * z_image / blur_partials are what ebos_blur3_variance_adjoint_f32 made of the IWE; the kernel reduces the partials (variance of the
 * blurred image -> out_variance / out_moments), and its upstream is a z + c wgt(pixel) with a = 2 upstream / (M - 1),
 * c = -a mean, wgt = B^T (valid region) evaluated from the pixel's position (csrc/blur3.h). */
int ebos_iwe_patch_tiled_bwd_blur_f32(const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt,
                                      const int32_t* key_offsets, int64_t n, const float* grid, int gh, int gw,
                                      int patch_h, int patch_w, int slide_h, int slide_w, int H, int W, int tile_h,
                                      int tile_w, int halo, int pad_h, int pad_w, const float* z_image, int g_lo,
                                      const float* upstream, float* grad_partials, size_t grad_partials_bytes,
                                      const int32_t* part_table, float w_flow_norm, float w_image_gradient,
                                      double* reg_partials, const double* blur_partials, int64_t n_blur_partials,
                                      int64_t n_var_pixels, float* out_variance, double* out_moments, float blur_k0,
                                      float blur_k1, ebos_stream_t stream);
/* The grid-sampling backward pass on a compact plan that carries the fractions of undistorted events (f64 sweep); blur_k0 == 0: the
 * plain contrast (g_image = the IWE, var_partials of the combine pass), else the blurred one (g_image = z_image, var_partials = the
 * blur pass's pairs) -- the arguments of the two entries above. */
int ebos_iwe_patch_tiled_bwd_frac_f32(const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt, const float* cfx, const float* cfy,
                                      const int32_t* key_offsets, int64_t n, const float* grid, int gh, int gw, int patch_h, int patch_w,
                                      int slide_h, int slide_w, int H, int W, int tile_h, int tile_w, int halo, int pad_h, int pad_w,
                                      const float* g_image, int g_lo, const double* var_moments, const float* upstream,
                                      const float* addend, float* grad_partials, size_t grad_partials_bytes, const int32_t* part_table,
                                      float w_flow_norm, float w_image_gradient, double* reg_partials, const double* var_partials,
                                      int64_t n_var_partials, int64_t n_var_pixels, float* out_variance, double* out_moments,
                                      float blur_k0, float blur_k1, ebos_stream_t stream);
/* ... and on the dense-flow route (windows of fractional source coordinates: the (x, y, dt) arrays; or compact ones): d loss / d flow
 * [2, H, W] of the blurred contrast, arguments as ebos_iwe_dense_tiled_bwd_f32 / ebos_iwe_patch_tiled_bwd_blur_f32. */
int ebos_iwe_dense_tiled_bwd_blur_f32(const float* xs, const float* ys, const float* dts, const int32_t* grp_offsets, const uint16_t* cpix,
                                      const float* cdt, const int32_t* key_offsets, int64_t n, const float* flow, int H, int W, int tile_h,
                                      int tile_w, int halo, int pad_h, int pad_w, const float* z_image, int g_lo, const float* upstream,
                                      const float* addend, float* d_flow, void* workspace, size_t workspace_bytes,
                                      const int32_t* part_table, const double* blur_partials, int64_t n_blur_partials,
                                      int64_t n_var_pixels, float* out_variance, double* out_moments, float blur_k0, float blur_k1,
                                      ebos_stream_t stream);
int ebos_patch_grad_combine_adam_f32(const float* grad_partials, const int32_t* part_table, int tile_h, int tile_w,
                                     int gh, int gw, int patch_h, int patch_w, int slide_h, int slide_w, int H, int W,
                                     float* d_grid, float* theta, float* exp_avg, float* exp_avg_sq, double lr,
                                     double beta1, double beta2, double eps, int t, int* step, const float* contrast,
                                     float contrast_scale, const double* reg_partials, int n_reg, float* losses,
                                     int losses_cap, const float* grad_mask, ebos_stream_t stream);

/* 2-DoF hypotheses on the tile-private pipeline (BASELINE config 5): thetas [K, 2] (device), x' = x + dt theta
 * (src/warp.py:364-383); iwes [K, h, w] are OVERWRITTEN; out_variance [K] / moments [K, 2] as above.  The K
 * hypotheses run back to back on the stream and share one workspace (same size as for the dense flow). */
int ebos_iwe_2dof_slab_f32(const float* xs, const float* ys, const float* dts, const float* weight,
                           const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt,
                           const int32_t* key_offsets, int64_t n, const float* thetas, int K,
                           int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w,
                           void* workspace, size_t workspace_bytes, float* iwes, int want_variance,
                           int omit_boundary, float* out_variance, double* moments, const int32_t* part_table,
                           ebos_stream_t stream);

/* The same K hypotheses with the accumulate pass PERSISTENT over them (the sweep of src/solver/generative_max_likelihood.py:229-255,
 * BASELINE config 5): one launch per 16 hypotheses in which every workgroup keeps its tile and walks the hypotheses -- one LDS
 * clear per launch, the decode pass zeroes what it reads, the next hypothesis' first chunks are requested while the current image
 * is decoded and stored -- followed by one combine and one finalize launch over (pixel block | 1, hypothesis).  Compact plans with
 * unit weights.  workspaces: K consecutive workspaces of workspace_bytes (>= ebos_iwe_slab_workspace_bytes, a multiple of 256) each,
 * zero-filled once; tail_stream (nullable) as in ebos_iwe_slab_batch_f32.  Results are bit-identical to ebos_iwe_2dof_slab_f32. */
int ebos_iwe_2dof_slab_batch_f32(const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt,
                                 const int32_t* key_offsets, int64_t n, const float* thetas, int K, int H, int W,
                                 int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w, void* workspaces,
                                 size_t workspace_bytes, float* iwes, int want_variance, int omit_boundary,
                                 float* out_variance, double* moments, const int32_t* part_table, ebos_stream_t stream,
                                 ebos_stream_t tail_stream);

/* backward of ebos_iwe_2dof_slab_f32: d_thetas[k] = sum_n dt * dL/d(x', y') for upstream images g_images [K, h, w]
 * (affine [K, 2] / g_lo as in ebos_iwe_dense_bwd_f32); d_thetas [K, 2] is OVERWRITTEN.  workspace: the plan's forward
 * workspace (its slab section is reused for the per-tile partial sums). */
int ebos_iwe_2dof_tiled_bwd_f32(const float* xs, const float* ys, const float* dts, const float* weight,
                                const int32_t* grp_offsets, const uint16_t* cpix, const float* cdt,
                                const int32_t* key_offsets, int64_t n, const float* thetas,
                                int K, int H, int W, int tile_h, int tile_w, int halo, int pad_h, int pad_w,
                                const float* g_images, const float* affine, int g_lo, float* d_thetas,
                                void* workspace, size_t workspace_bytes, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused hot path, 2-DoF hypotheses (solver outer loop, SURVEY.md 3.4 / BASELINE config 5):
 *   A4 + A7 for K translations theta[k] = (theta0, theta1) in one pass over the events
 *   (src/warp.py:364-383 + src/event_image_converter.py:581-620).  iwes [K, h, w] accumulates.
 *   bwd: d_theta[k][c] += sum_n dt * dL/d(x',y') for upstream images g [K, h, w].
 * ---------------------------------------------------------------------------------------- */
int ebos_iwe_2dof_f32(const float* x, const float* y, const float* dt, const float* weight, int64_t n,
                      const float* thetas, int K, int h, int w, int pad_h, int pad_w, float* iwes,
                      ebos_stream_t stream);
int ebos_iwe_2dof_bwd_f32(const float* x, const float* y, const float* dt, const float* weight, int64_t n,
                          const float* thetas, int K, int h, int w, int pad_h, int pad_w,
                          const float* g_images, const float* affine, int g_lo, float* d_thetas,
                          ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A14  contrast costs on an image (absent from the release; defined in SURVEY.md A14 on the
 *      reference's primitives torch.var and SobelTorch, src/utils/stat_utils.py:48-139;
 *      dict keys "iwe"/"omit_boundary" per src/solver/base.py:337-339).
 *   images [K, h, w]; omit_boundary crops one pixel on every side (iwe[..., 1:-1, 1:-1]).
 *   variance:            out[k] = unbiased variance;  moments[k] = {mean, M} (f64, nullable)
 *   gradient magnitude:  out[k] = mean(gx^2 + gy^2), (gx, gy) = Sobel3(replicate pad) / 8
 *   *_grad: d_images[k] = upstream[k] * d(out[k]) / d(image[k])  (overwrites; upstream device [K], f32)
 *   Sums are carried in f64.  scratch: >= ebos_cost_scratch_bytes(K) bytes.
 * ---------------------------------------------------------------------------------------- */
size_t ebos_cost_scratch_bytes(int K);
int ebos_image_variance_f32(const float* images, int K, int h, int w, int omit_boundary, float* out,
                            double* moments, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_image_variance_grad_f32(const float* images, int K, int h, int w, int omit_boundary,
                                 const double* moments, const float* upstream, float* d_images,
                                 ebos_stream_t stream);
/* (a, c) per image such that d(out)/d(image) * upstream = a * image + c inside the valid region:
 * feeds ebos_iwe_*_bwd_f32's `affine` without materialising d_images.  affine [K, 2] f32. */
int ebos_image_variance_affine_f32(const double* moments, const float* upstream, int K, float* affine,
                                   ebos_stream_t stream);
int ebos_gradient_magnitude_f32(const float* images, int K, int h, int w, int omit_boundary, float* out,
                                void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_gradient_magnitude_grad_f32(const float* images, int K, int h, int w, int omit_boundary,
                                     const float* upstream, float* d_images, ebos_stream_t stream);
int ebos_image_variance_f64(const double* images, int K, int h, int w, int omit_boundary, double* out,
                            double* moments, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_image_variance_grad_f64(const double* images, int K, int h, int w, int omit_boundary,
                                 const double* moments, const double* upstream, double* d_images,
                                 ebos_stream_t stream);
int ebos_gradient_magnitude_f64(const double* images, int K, int h, int w, int omit_boundary, double* out,
                                void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_gradient_magnitude_grad_f64(const double* images, int K, int h, int w, int omit_boundary,
                                     const double* upstream, double* d_images, ebos_stream_t stream);
/* Value AND gradient image of the gradient-magnitude contrast in ONE pass over an LDS-tiled image (the two entry points above read
 * the image twice, the second one 81 times per pixel): out[0] = mean(gx^2 + gy^2) with (gx, gy) = Sobel 3x3 / 8, replicate padding
 * (src/utils/stat_utils.py:69-92, 117-139), d_image [h, w] = upstream[0] * d out / d image (upstream: device f32 [1], NULL = 1) --
 * the bits of ebos_gradient_magnitude_grad_f32.  partials: device f64 [ebos_gradient_magnitude_fused_partials(h, w)], one value
 * partial per workgroup; out == NULL: no finalize launch (the caller sums the partials: ebos_gradient_magnitude_dense_job_f32);
 * d_image == NULL (with out != NULL): the value only -- no gather of the stencils, no gradient image written. */
int64_t ebos_gradient_magnitude_fused_partials(int h, int w);
int ebos_gradient_magnitude_fused_f32(const float* image, int h, int w, int omit_boundary, const float* upstream, float* out,
                                      float* d_image, double* partials, int64_t n_partials, ebos_stream_t stream);

/* Variance of the 3-tap blurred image y = B x -- torchvision gaussian_blur(kernel_size = 3): taps (k0, k1, k0) =
 * exp(-x^2 / 2 sigma^2) at x = -1, 0, 1 normalised to sum 1, reflect padding without edge repeat,
 * src/event_image_converter.py:399-404 -- prepared for the solver loop in ONE pass over the image: partials
 * [ebos_blur3_variance_partials(h, w)][2] f64 = (sum, sum of squares) of the valid blurred pixels per 16 x 64 tile (the layout of
 * the slab combine pass's partials), and z_image [h, w] = B^T (m . y), the part of d var(y) / d x that is linear in x
 * (m = the valid region, omit_boundary).  h, w >= 2 (torch refuses to reflect-pad an axis of one sample). */
int64_t ebos_blur3_variance_partials(int h, int w);
/* cost_scratch of ebos_cmax_patch_problem / ebos_cmax_2dof_problem for an image of h x w pixels (padding included): enough for the
 * value partials of the fused Sobel pass (w_gradient_magnitude != 0) and for the blur's partial pairs (blur_k0 != 0).  ABI 2:
 * ebos_cost_scratch_bytes(1), which ABI 1 documented for this buffer, is too small for the Sobel partials of images beyond ~0.5 MP. */
size_t ebos_cmax_cost_scratch_bytes(int h, int w);
int ebos_blur3_variance_adjoint_f32(const float* image, int h, int w, int omit_boundary, float k0, float k1, float* z_image,
                                    double* partials, int64_t n_partials, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A16  patch grid -> dense flow  (src/solver/patch_eklt.py:173-204): replicate-pad the grid by
 *      pad = int(patch/2 // slide) + 1, bilinear resize (align_corners = False) by the sliding
 *      window, centre-crop to [H, W].  grid [2, gh, gw] -> dense [2, H, W] (overwrites).
 *      bwd: the adjoint, as two separable passes through a [2, gh, W] scratch.
 * ---------------------------------------------------------------------------------------- */
int ebos_upsample_patch_flow_f32(const float* grid, int gh, int gw, int patch_h, int patch_w, int slide_h,
                                 int slide_w, int H, int W, float* dense, ebos_stream_t stream);
/* adjoint: d_grid [2, gh, gw] is OVERWRITTEN.  scratch: device, ebos_upsample_bwd_scratch_bytes(gh, W). */
size_t ebos_upsample_bwd_scratch_bytes(int gh, int W);
int ebos_upsample_patch_flow_bwd_f32(const float* d_dense, int gh, int gw, int patch_h, int patch_w,
                                     int slide_h, int slide_w, int H, int W, float* scratch, float* d_grid,
                                     ebos_stream_t stream);
/* The same adjoint with the Adam step of the patch grid applied where each gradient element is produced (Adam is
 * element-wise): theta / exp_avg / exp_avg_sq [2, gh, gw] are updated in place with the gradient of step t (t >= 1,
 * counted by the caller; bias corrections in double on the host like torch.optim.Adam), d_grid still receives the
 * gradient, step[0] := t, and losses[t - 1] := contrast_scale * contrast[0] + sum(reg_partials) (the loss of the
 * parameters before the update; contrast / reg_partials / losses nullable).  Replaces ebos_upsample_patch_flow_bwd_f32 +
 * ebos_cmax_adam_step_f32 in the solver loop: one launch less per iteration.
 * grad_mask [gh, gw] (nullable) multiplies the gradient of both flow components before the step: 0 for the patches that
 * are not estimated -- the event thresholding of src/solver/patch_eklt.py:118-126 (`len(crop_event(...)) > event_thres`),
 * whose patch flow stays where it is (Adam with a zero gradient and zero moments does not move). */
int ebos_upsample_patch_flow_bwd_adam_f32(const float* d_dense, int gh, int gw, int patch_h, int patch_w,
                                          int slide_h, int slide_w, int H, int W, float* scratch, float* d_grid,
                                          float* theta, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                                          double beta2, double eps, int t, int* step, const float* contrast,
                                          float contrast_scale, const double* reg_partials, int n_reg, float* losses,
                                          int losses_cap, const float* grad_mask, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A9/K11  optional Gaussian blur of an event image (sigma > 0), one separable pass along one axis
 *     of a tensor viewed as [outer, L, inner]; taps: device [2 radius + 1] doubles (host-computed).
 *     boundary 0 = scipy 'reflect' (d c b a | a b c d): gaussian_filter(image, sigma) of the numpy
 *                  branch, one pass per array axis  (src/event_image_converter.py:368-369);
 *     boundary 1 = torch 'reflect' (d c b | a b c d): torchvision gaussian_blur(kernel_size=3) of the
 *                  tensor branch, last two axes     (src/event_image_converter.py:399-404).
 *     out must not alias in.
 * ---------------------------------------------------------------------------------------- */
int ebos_gauss1d_f32(const float* in, float* out, int64_t outer, int64_t L, int64_t inner, const double* taps,
                     int radius, int boundary, ebos_stream_t stream);
int ebos_gauss1d_f64(const double* in, double* out, int64_t outer, int64_t L, int64_t inner, const double* taps,
                     int radius, int boundary, ebos_stream_t stream);
/* Adjoint of one pass: g_in = (d loss / d in) from g_out = (d loss / d out).  What torch autograd
 * derives for gaussian_blur in the tensor branch (src/event_image_converter.py:399-404); gather
 * form, deterministic.  g_in must not alias g_out. */
int ebos_gauss1d_bwd_f32(const float* g_out, float* g_in, int64_t outer, int64_t L, int64_t inner,
                         const double* taps, int radius, int boundary, ebos_stream_t stream);
int ebos_gauss1d_bwd_f64(const double* g_out, double* g_in, int64_t outer, int64_t L, int64_t inner,
                         const double* taps, int radius, int boundary, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One contrast-maximisation iteration without autograd glue.  The loop of
 * src/solver/generative_max_likelihood.py:306-341 (zero_grad -> objective -> backward -> Adam step)
 * becomes 5 calls / 8 kernels on one stream (7 without regularisers + 1 finalize):
 *     ebos_upsample_patch_flow_f32 -> ebos_iwe_dense_slab_f32 (want_variance) -> ebos_flow_regularisers_f32
 *     -> ebos_iwe_dense_tiled_bwd_f32 (var_moments, upstream = -weight, addend = regulariser gradient)
 *     -> ebos_upsample_patch_flow_bwd_adam_f32   (ebos_cmax_adam_step_f32 is the stand-alone form of the step)
 *
 * ebos_flow_regularisers_f32: value and gradient of
 *       w_flow_norm * mean_px |flow|_2                                   (src/costs/flow_norm.py:45-56)
 *     + w_image_gradient * mean(|d flow/d row| + |d flow/d col|)         (src/costs/image_gradient.py:60-75,
 *                                                                         torch.gradient, unit weights)
 *   flow [2, H, W]; d_flow [2, H, W] is OVERWRITTEN with the gradient; partials: device doubles,
 *   ebos_flow_regularisers_partials() of them, whose sum is the value (ebos_cmax_adam_step sums them).
 *   var_partials (nullable) .. moments: a side job for one of its workgroups -- reduce the variance partials that
 *   ebos_iwe_dense_slab_f32(want_variance = 2) left in its workspace (ebos_iwe_slab_partials locates them) into
 *   out_variance / moments, instead of a finalize launch of its own.
 * ebos_cmax_adam_step_f32: torch.optim.Adam (amsgrad off, no weight decay) on theta[n] given grad[n],
 *   with state exp_avg[n], exp_avg_sq[n] and a device step counter step[1] (all zero-initialised by the
 *   caller); records losses[step] = contrast_scale * contrast[0] + sum(reg_partials) for the parameters
 *   BEFORE the update (contrast / reg_partials / losses nullable) and increments step.  One workgroup.
 * ---------------------------------------------------------------------------------------- */
int ebos_flow_regularisers_partials(void);
int ebos_flow_regularisers_f32(const float* flow, int H, int W, float w_flow_norm, float w_image_gradient,
                               float* d_flow, double* partials, const double* var_partials, int64_t n_var_partials,
                               int64_t n_var_pixels, float* out_variance, double* moments, ebos_stream_t stream);
int ebos_cmax_adam_step_f32(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, int n, double lr,
                            double beta1, double beta2, double eps, int* step, const float* contrast,
                            float contrast_scale, const double* reg_partials, int n_reg, float* losses,
                            int losses_cap, ebos_stream_t stream);

/* The whole loop natively: n_iter iterations of the six calls above, enqueued back to back on `stream` by one
 * C call (no interpreter between launches; asynchronous like everything else).  All buffers are the caller's:
 *   plan:     xs/ys/dts (nullable when the compact trio is given), grp_offsets/cpix/cdt, key_offsets, n, H, W, tile,
 *             halo, pad, omit_boundary, splits, part_table -- as ebos_iwe_dense_slab_f32 / ebos_iwe_dense_tiled_bwd_f32
 *   grid:     theta/d_theta/exp_avg/exp_avg_sq [2, gh, gw], step [1] int32, patch and sliding window
 *   images:   dense/d_dense [2, H, W], d_reg [2, H, W] (nullable iff both regulariser weights are 0),
 *             iwe [H + 2 pad_h, W + 2 pad_w], variance [1] f32, moments [2] f64, upstream [1] f32 = -w_variance
 *   scratch:  reg_partials [max(ebos_flow_regularisers_partials(), work items = ebos_patch_grad_partials_bytes / 2048)] f64,
 *             zero-filled once; upsample_scratch
 *             (ebos_upsample_bwd_scratch_bytes), workspace (ebos_iwe_slab_workspace_bytes, zero-filled once)
 *   losses:   [losses_cap] f32, entry `step` written per iteration (nullable)
 *   theta_mask: [gh, gw] f32, 0 = patch not estimated (nullable = all patches)                                 */
typedef struct ebos_cmax_patch_problem {
  const float *xs, *ys, *dts;
  const int32_t* grp_offsets;
  const uint16_t* cpix;
  const float* cdt;
  const int32_t* key_offsets;
  int64_t n;
  int H, W, tile_h, tile_w, halo, pad_h, pad_w, omit_boundary;
  int splits;                  /* as ebos_iwe_dense_slab_f32; 0 = adaptive work items of part_table */
  const int32_t* part_table;   /* nullable unless splits == 0 */
  int gh, gw, patch_h, patch_w, slide_h, slide_w;
  float w_variance, w_flow_norm, w_image_gradient;
  float w_gradient_magnitude;  /* contrast = gradient magnitude instead of variance: exactly one of the two
                                  contrast weights is non-zero; then `variance` receives the contrast value, `upstream` holds
                                  -w_gradient_magnitude, and d_iwe / cost_scratch below are needed */
  double lr, beta1, beta2, eps;
  float *theta, *d_theta, *exp_avg, *exp_avg_sq;
  int* step;
  int steps_done;              /* Adam steps already applied to theta (the first iteration of a solve is step steps_done + 1) */
  float *dense, *d_dense, *d_reg, *iwe, *variance;
  float* d_iwe;                /* [H + 2 pad_h, W + 2 pad_w]; nullable unless w_gradient_magnitude != 0 */
  void* cost_scratch;          /* >= ebos_cmax_cost_scratch_bytes(H + 2 pad_h, W + 2 pad_w) (the fused Sobel pass's value partials / the
                                  blur's partial pairs); nullable unless w_gradient_magnitude != 0 or blur_k0 != 0 */
  size_t cost_scratch_bytes;
  double* moments;
  const float* upstream;
  double* reg_partials;
  float* upsample_scratch;
  void* workspace;
  size_t workspace_bytes;
  float* losses;
  int losses_cap;
  const float* theta_mask;     /* [gh, gw], nullable: grad_mask of ebos_upsample_patch_flow_bwd_adam_f32 */
  float* grad_partials;        /* non-NULL: the event kernels sample the patch grid themselves (ebos_iwe_patch_*; needs
                                  ebos_patch_fused_supported and the compact plan); dense / d_dense / d_reg / upsample_scratch are
                                  then not used (the backward kernel evaluates the flow regularisers from the tile's flow) */
  size_t grad_partials_bytes;  /* ebos_patch_grad_partials_bytes(H, W, tile_h, tile_w, splits == 0) */
  /* ABI 2: iwe.blur_sigma > 0 -- the variance is taken on the 3-tap blurred IWE (src/event_image_converter.py:399-404).
   * blur_k0 = 0: no blur.  Otherwise the taps (blur_k0, blur_k1, blur_k0), blur_image [H + 2 pad_h, W + 2 pad_w] and cost_scratch
   * >= 16 * ebos_blur3_variance_partials(H + 2 pad_h, W + 2 pad_w) bytes; the variance contrast only. */
  float blur_k0, blur_k1;
  float* blur_image;
  /* the resident launch on a window of FRACTIONAL source coordinates (sub-pixel rectified or pre-warped events):
   * with cfx / cfy non-NULL, grp_offsets / cpix / cdt / cfx / cfy are the arrays of ebos_plan_compact_frac_f32.  The resident launch
   * reads them, and so does the four-launch loop when grad_partials is given (grid-sampling route on the fractions: general event
   * loops); with grad_partials NULL the launches run the dense route on xs / ys / dts. */
  const float *cfx, *cfy;
} ebos_cmax_patch_problem;
int ebos_cmax_patch_solve_f32(const ebos_cmax_patch_problem* problem, int n_iter, ebos_stream_t stream);
/* ebos_cmax_patch_gradient_f32: one forward and backward at theta without the Adam step -- d_theta, variance (the contrast value),
 *   moments and reg_partials are left for the caller (loss = -(w_variance or w_gradient_magnitude) * variance[0] + sum of the first
 *   n reg_partials, n = ebos_flow_regularisers_partials() on the dense route, grad_partials_bytes / 2048 with grad_partials, 0 without
 *   a regulariser weight); for optimisers that live on the host.  The same checks and the same launches as one iteration of
 *   ebos_cmax_patch_solve_f32 up to the finishing call, which is the plain adjoint (ebos_patch_grad_combine_adam_f32 with theta = NULL,
 *   or ebos_upsample_patch_flow_bwd_f32): theta, exp_avg, exp_avg_sq, step and losses are not written, theta_mask is not applied.
 *   blur_k0 != 0 is refused (EBOS_ERR_UNSUPPORTED): the blurred contrast is part of the Adam loop only. */
int ebos_cmax_patch_gradient_f32(const ebos_cmax_patch_problem* problem, ebos_stream_t stream);
/* Several independent windows at once (windows are the unit that shards): problem w runs on
 * streams[w]; launches are enqueued iteration-major so that the windows' kernels interleave on the GPU. */
int ebos_cmax_patch_solve_many_f32(const ebos_cmax_patch_problem* problems, const ebos_stream_t* streams,
                                   int n_problems, int n_iter);

/* The Adam loop of the 2-DoF motion model natively (motion_model "2d-translation" with optimizer Adam, n_iter 600 and
 * iwe.blur_sigma 3 is what configs/hot_plate1.yaml:47,65,70 selects; loop: src/solver/generative_max_likelihood.py:306-341):
 *     loss(theta) = -w_variance * var([blur3] IWE(x + dt theta)),   theta = (trans_x, trans_y)   (src/warp.py:364-383)
 * n_iter iterations enqueued by one C call, four launches each (five with the blur), no host synchronisation.
 *   plan:    xs / ys / dts and / or the compact trio (grp_offsets / cpix / cdt), key_offsets, tile, halo, pad, omit_boundary,
 *            splits, part_table as ebos_iwe_2dof_slab_f32
 *   state:   theta / d_theta / exp_avg / exp_avg_sq [2] f32, step [1] int32; steps_done = Adam steps already applied
 *   images:  iwe [H + 2 pad_h, W + 2 pad_w]; blur_image of the same shape and cost_scratch >= 16 * ebos_blur3_variance_partials
 *            bytes when blur_k0 != 0 (taps blur_k0, blur_k1, blur_k0)
 *   scalars: variance [1] f32 and moments [2] f64 receive the contrast of the last iteration; upstream [1] f32 = -w_variance
 *   losses:  [losses_cap] f32, entry `step` written per iteration with the loss BEFORE the update (nullable) */
typedef struct ebos_cmax_2dof_problem {
  const float *xs, *ys, *dts;  /* the plan's (x, y, dt) arrays: needed when the compact trio is NULL (fractional -- undistorted --
                                  source coordinates), else nullable */
  const int32_t* grp_offsets;
  const uint16_t* cpix;
  const float* cdt;
  const float *cfx, *cfy;      /* compact plan of FRACTIONAL source coordinates (ebos_plan_compact_frac_f32): x - floor(x), y - floor(y)
                                  per slot, laid out like cdt; both or neither (else EBOS_ERR_INVALID_ARG; ..._resident_supported says 0); NULL = integer
                                  source pixels.  Read by BOTH forms of the loop: ebos_cmax_2dof_solve_f32's launches take the compact
                                  trio + cfx / cfy when they are given and xs / ys / dts only when the trio is NULL */
  const int32_t* key_offsets;
  int64_t n;
  int H, W, tile_h, tile_w, halo, pad_h, pad_w, omit_boundary;
  int splits;
  const int32_t* part_table;
  float w_variance;            /* > 0; the device word `upstream` below holds -w_variance (the four launches read the device word, the
                                  resident launch the host value) */
  float blur_k0, blur_k1;
  double lr, beta1, beta2, eps;
  float *theta, *d_theta, *exp_avg, *exp_avg_sq;
  int* step;
  int steps_done;
  float *iwe, *blur_image, *variance;
  double* moments;
  const float* upstream;
  void* cost_scratch;
  size_t cost_scratch_bytes;
  void* workspace;
  size_t workspace_bytes;
  float* losses;
  int losses_cap;
} ebos_cmax_2dof_problem;
int ebos_cmax_2dof_solve_f32(const ebos_cmax_2dof_problem* problem, int n_iter, ebos_stream_t stream);


/* ---- the same loop as ONE resident launch (csrc/cmax_resident.hip) -------------------------------------------------------------
 * Replaces, for one window, the n_iter x 4 launches that ebos_cmax_patch_solve_f32 enqueues for the loop of
 * src/solver/generative_max_likelihood.py:306-341 (600 iterations over the SAME events, configs/hot_plate1.yaml:70): one
 * 1024-thread workgroup per source tile stays resident for all iterations, keeps its tile's geometry, grid cells and Adam state
 * in registers / LDS, and exchanges only slabs, (sum, sum of squares) records and partial cell gradients with its neighbours
 * through `workspace`, `grad_partials` and `mailbox`.  Same `problem` struct, same results (IWE bit-identical; losses to ~1e-7).
 *
 *   ebos_cmax_resident_supported   1 when `problem` can run resident: a compact plan -- of the grid-sampling route (grad_partials), or
 *                                  with the fractions of undistorted events (cfx / cfy) --, either contrast (the blurred image with
 *                                  the variance only), splits 0 or 1, image padding below half a tile and at most the halo (round 6: the windows
 *                                  then reach at least the padding ring), tile / halo with a resident kernel ((45, 80, 32),
 *                                  (32, 32, 32), (32, 64, 32)), cell blocks of <= 256 elements per tile, cells whose supports span
 *                                  <= 16 tiles per axis; 0 otherwise (reason: ebos_last_error)
 *   mailbox                        device memory of ebos_cmax_resident_mailbox_bytes(...): flags, records, the status word;
 *                                  cleared by every call
 *   spin_timeout_s                 cap of every in-kernel wait (seconds; e.g. 2.0).  The grid must be co-resident -- the call
 *                                  checks tiles <= CUs x occupancy and orders resident launches of one device behind each other --
 *                                  but if a wait still passes the cap (another process's resident grid interleaved with this
 *                                  one), or a tap leaves the largest LDS window (the spill path of the four-launch pipeline),
 *                                  the launch ENDS instead of hanging and leaves theta / exp_avg / exp_avg_sq / step untouched --
 *                                  except after a spill in iteration k >= 1, when it hands over the state of its k completed
 *                                  iterations (ebos_cmax_resident_iterations = k; continue with ebos_cmax_patch_solve_f32 and
 *                                  steps_done + k).  The first verdict of a launch stands; should its workgroups have left on
 *                                  two different ones, ebos_cmax_resident_iterations returns -1: the state is partly written.
 *   ebos_cmax_resident_status      synchronises `stream`, returns EBOS_OK or a negative code (-101 spin cap, -102 spill,
 *                                  -103 geometry, -104 a crowded window: on a sensor of >= 128 tiles the fullest tile holds more
 *                                  than 60 k + 0.8 % of the window's events, on smaller ones more than 85 k -- the kernel's own
 *                                  verdict in its first iteration; EBOS_RESIDENT_MAX_IMBALANCE = r > 0: more than r x the average
 *                                  tile's events (and >= 32 k), or >= 120 k and more than r / 4 x; 0 = never); on a negative code run
 *                                  ebos_cmax_patch_solve_f32 with the same problem.  -102 is also how the blurred and the
 *                                  gradient-magnitude loops hand over when the windows outgrow their LDS regions (~12 px).  */
size_t ebos_cmax_resident_mailbox_bytes(int H, int W, int tile_h, int tile_w);
int ebos_cmax_resident_supported(const ebos_cmax_patch_problem* problem);
int ebos_cmax_patch_solve_resident_f32(const ebos_cmax_patch_problem* problem, int n_iter, void* mailbox, size_t mailbox_bytes,
                                       double spin_timeout_s, ebos_stream_t stream);
/* The 2-DoF Adam loop (ebos_cmax_2dof_solve_f32) as ONE resident launch: same problem struct, same mailbox / spin cap / status
 * protocol as ebos_cmax_patch_solve_resident_f32 (ebos_cmax_resident_status / _iterations read its mailbox too).  Compact plans,
 * splits <= 1, image padding below half a tile, the tiles (45, 80) / (32, 32) / (32, 64) with halo 32.  Every workgroup sums all tiles' partial pairs of
 * d loss / d theta itself and steps the two parameters redundantly; with blur_k0 != 0 the gathered window is blurred in LDS
 * (windows up to ~12 px; larger displacements hand over with -102 like a spill). */
int ebos_cmax_2dof_resident_supported(const ebos_cmax_2dof_problem* problem);
int ebos_cmax_2dof_solve_resident_f32(const ebos_cmax_2dof_problem* problem, int n_iter, void* mailbox, size_t mailbox_bytes,
                                      double spin_timeout_s, ebos_stream_t stream);
int ebos_cmax_resident_status(const void* mailbox, ebos_stream_t stream);
/* The iterations the launch completed (synchronises `stream`): n_iter after status 0; after -102 (a tap left the largest LDS
 * window in iteration k >= 1) the k iterations before it -- theta, the optimiser state, the step counter and the losses are then
 * those of k iterations and ebos_cmax_patch_solve_f32 continues with the remaining n_iter - k; 0 after any other negative status
 * (nothing changed). */
int ebos_cmax_resident_iterations(const void* mailbox, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Event filters (src/utils/event_filters.py), bit-identical to the reference's per-event loops.
 *
 * A window is described by an ebos_event_source (host struct, device buffers):
 *   kind EBOS_FILTER_SRC_F32 / _F64: AoS events [n, 4]; `layout` = ix | iy << 2 | it << 4 names the row, column and
 *        time columns (index_convention, :21; the default (0, 1, 2) is layout 0x24); pixels are int(x), int(y) of
 *        the input's own dtype (truncation), times the input's values as float64;
 *   kind EBOS_FILTER_SRC_RAW32 / _RAW64: raw sensor columns col (= y) / row (= x) int16, t int32 / int64 ticks,
 *        pol uint8 (compaction only); t in seconds = (double)t / ticks_per_second (data_loader.py:104).
 * A filter reads the events with mask_in[i] != 0 (mask_in NULL = all n) and writes mask_out[n] (1 = kept, 0 otherwise)
 * and the kept count *n_out (device int32).  n_in (device int32, nullable) is the number of events in the filter's input:
 * when it is below 10 the filter is skipped -- mask_out = mask_in, *n_out = *n_in, time map unchanged -- as
 * EventFilter.process skips the remaining filters (:184-187), so that a chain of filters runs without a host read-back.
 * status[3] (device int32, accumulates; the caller zeroes it): [EBOS_FILTER_STATUS_OUT_OF_SENSOR] input events whose
 * pixel lies outside [0, H) x [0, W) (the reference wraps negative indices; callers raise), [EBOS_FILTER_STATUS_CLIPPED]
 * events whose clipped BAF neighbourhood holds fewer than num_support_event + 1 pixels (the reference raises IndexError
 * at time_array[-1 - num_support_event], :89).  Outputs are undefined when either is non-zero.
 * scratch: ebos_event_filter_scratch_bytes(n, H, W) bytes (caller-owned) for any of the three calls.
 *
 *   ebos_baf_mask        continuous_background_activity_filter (:46-97): events in array order, time map
 *                        M = time_map_in ([H, W] float64; NULL = zeros) updated to max(M, t) at the event's pixel, kept iff
 *                        t - (the (num_support_event + 1)-th largest M over the clipped (2 ksize + 1)^2 neighbourhood) < dt;
 *                        the final map -> time_map_out (may be time_map_in).  0 <= ksize <= 7 and
 *                        0 <= num_support_event <= 15, else EBOS_ERR_UNSUPPORTED.  Deterministic: no atomic order
 *                        reaches any output.
 *   ebos_hot_mask        hot_pixel_filter (:100-128): drops the events of pixels whose image value is > thresh.  iwe NULL:
 *                        the value is the pixel's event count (= create_iwe(events, sigma=0) for integer coordinates);
 *                        else iwe [H, W] float64 of the input events (ebos_splat_f64, bilinear, eps 1e-8: fractional
 *                        coordinates).
 *   ebos_filter_compact  the events with mask[i] != 0, in their order, in the source's own format -> events_out [n, 4]
 *                        (AoS) or col_out / row_out / t_out / pol_out (raw); *n_out = their number (replaces the
 *                        np.vstack of kept events, :95-97, 128).
 * ---------------------------------------------------------------------------------------- */
typedef enum ebos_filter_source_kind {
  EBOS_FILTER_SRC_F32 = 0,
  EBOS_FILTER_SRC_F64 = 1,
  EBOS_FILTER_SRC_RAW32 = 2,
  EBOS_FILTER_SRC_RAW64 = 3
} ebos_filter_source_kind;

typedef enum ebos_filter_status_slot {
  EBOS_FILTER_STATUS_OUT_OF_SENSOR = 0,
  EBOS_FILTER_STATUS_CLIPPED = 1
} ebos_filter_status_slot;

typedef struct ebos_event_source {
  int kind, layout;
  const void* events;
  const int16_t* col;
  const int16_t* row;
  const void* t;
  const uint8_t* pol;
  double ticks_per_second;
  int64_t n;
} ebos_event_source;

size_t ebos_event_filter_scratch_bytes(int64_t n, int H, int W);
int ebos_baf_mask(const ebos_event_source* src, int H, int W, const uint8_t* mask_in, const int32_t* n_in, double dt, int ksize,
                  int num_support_event, const double* time_map_in, double* time_map_out, uint8_t* mask_out, int32_t* n_out,
                  int32_t* status, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_hot_mask(const ebos_event_source* src, int H, int W, const uint8_t* mask_in, const int32_t* n_in, double thresh,
                  const double* iwe, uint8_t* mask_out, int32_t* n_out, int32_t* status, void* scratch, size_t scratch_bytes,
                  ebos_stream_t stream);
int ebos_filter_compact(const ebos_event_source* src, const uint8_t* mask, void* events_out, int16_t* col_out, int16_t* row_out,
                        void* t_out, uint8_t* pol_out, int32_t* n_out, void* scratch, size_t scratch_bytes, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Flow-error metrics (src/utils/flow_utils.py:706-823, calculate_flow_error_tensor / calculate_flow_error_numpy) for a
 * batch of B flows [B, 2, H, W] in one call:
 *   flow_mask = !isinf(gt_u) & !isinf(gt_v) & |gt_u| > 0 & |gt_v| > 0, total = flow_mask & (event_mask != 0);
 *   g = gt * total, p = pred * total (multiplied: NaN / inf anywhere gives NaN sums, as in the reference), both times
 *   time_scale[b] when time_scale is non-NULL; e = sqrt(dx * dx + dy * dy) of d = g - p; n = count(total) + 1e-5;
 *   EPE = sum(e) / n, kPE = count(e > k) / n for k in {1, 2, 3, 5, 10, 20},
 *   AE = sum(acos((1 + u u_gt + v v_gt) / (sqrt(1 + u u + v v) sqrt(1 + u_gt u_gt + v_gt v_gt)))) / n.
 * The reference's IEEE operations in its order, uncontracted, correctly rounded sqrt: float64 e is bit-equal to numpy's.
 * float32 flows are masked, scaled and differenced in float32; the norm, the AE term and all sums are float64.
 *
 * dtype: EBOS_FLOW_ERROR_F32 / _F64, the element type of flow_gt, flow_pred and time_scale ([B], nullable).
 * Strides are in elements (batch, channel, row); columns are unit-stride, so an ROI view is read in place.  event_mask
 * (nullable: no event mask) is uint8 [B, H, W] with strides (mask_sb, mask_sr) and unit column stride; any non-zero byte
 * is true; mask_sb = 0 broadcasts one mask over the batch.  flags: EBOS_FLOW_ERROR_CLAMP_AE clamps the AE cosine to
 * [-1, 1] (not the reference, whose AE is NaN when rounding pushes it above 1, e.g. for pred == gt).
 * out: device double [(B + 1) * 9], per item EPE, 1PE, 2PE, 3PE, 5PE, 10PE, 20PE, AE, count(total), then one row of the
 * means over the batch.  scratch: ebos_flow_error_scratch_bytes(B, H, W) bytes (caller-owned).  Three launches, no
 * atomics: bit-identical from run to run.  0 < B <= 65535 and H * W < 2^31, else EBOS_ERR_INVALID_ARG.
 * ---------------------------------------------------------------------------------------- */
typedef enum ebos_flow_error_dtype {
  EBOS_FLOW_ERROR_F32 = 0,
  EBOS_FLOW_ERROR_F64 = 1
} ebos_flow_error_dtype;

#define EBOS_FLOW_ERROR_CLAMP_AE 1

size_t ebos_flow_error_scratch_bytes(int B, int H, int W);
int ebos_flow_error(int dtype, int B, int H, int W, const void* flow_gt, int64_t gt_sb, int64_t gt_sc, int64_t gt_sr,
                    const void* flow_pred, int64_t pred_sb, int64_t pred_sc, int64_t pred_sr, const uint8_t* event_mask,
                    int64_t mask_sb, int64_t mask_sr, const void* time_scale, int flags, double* out, void* scratch,
                    size_t scratch_bytes, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Poisson integration of BOS flows (src/utils/stat_utils.py:142-199, poisson_reconstruct, and the uint8 picture of
 * src/visualizer.py:419-435) for a batch of B flows [B, 2, H, W] (component 0 = gradx, 1 = grady) in one call:
 *   F = interior divergence (gx[i, j] - gx[i, j-1]) + (gy[i, j] - gy[i-1, j]), differences in in_dtype, sum in float64, minus the
 *       5-point stencil of the boundary with its interior zeroed (in out_dtype);
 *   P = S_h^T ((S_h F S_w^T) / D) S_w on the (H-2) x (W-2) interior, S_N the orthonormal DST-II matrix, D the eigenvalues of the
 *       5-point Laplacian; out = the boundary with its interior replaced by P (zeros + P without a boundary).
 * Four fp64 MFMA GEMMs, float64 throughout; no atomics, no split-K: an item's bits do not depend on B or on the run.
 *
 * in_dtype: EBOS_POISSON_F32 / _F64, the element type of flow (element strides flow_sb, flow_sc, flow_sr; unit columns).
 * out_dtype: the element type of boundary (nullable = zeros; strides bnd_sb -- 0 broadcasts one boundary --, bnd_sr) and of out
 * ([B, H, W], strides out_sb, out_sr).  out_u8 (nullable): device uint8 [B, H, W] contiguous, trunc(P / max|P| * 127 + 128) in
 * out_dtype (the reference's standardize_image_center(P).astype(np.uint8)); all-zero P gives 128.  scratch:
 * ebos_poisson_scratch_bytes(B, H, W) bytes, 16-byte aligned (caller-owned).  H, W >= 3, H * W < 2^31, B <= 65535, else
 * EBOS_ERR_INVALID_ARG; a short scratch is EBOS_ERR_SCRATCH.
 * ---------------------------------------------------------------------------------------- */
typedef enum ebos_poisson_dtype {
  EBOS_POISSON_F32 = 0,
  EBOS_POISSON_F64 = 1
} ebos_poisson_dtype;

size_t ebos_poisson_scratch_bytes(int B, int H, int W);
int ebos_poisson_reconstruct(int in_dtype, int out_dtype, int B, int H, int W, const void* flow, int64_t flow_sb, int64_t flow_sc,
                             int64_t flow_sr, const void* boundary, int64_t bnd_sb, int64_t bnd_sr, void* out, int64_t out_sb,
                             int64_t out_sr, uint8_t* out_u8, void* scratch, size_t scratch_bytes, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Dense optical flow between frame pairs: OpenCV's calcOpticalFlowFarneback with flags 0, the frame-based flow of the reference
 * (src/frame_flow_estimator.py:30-95 -> src/utils/frame_utils.py:160-183), for B pairs (prev[b], next[b]) in one call.
 *   per level k = levels' .. 0 (levels' cut where a side of the frame times pyr_scale^k falls below 32 pixels): both frames
 *   converted to float32, Gaussian-blurred at full resolution (sigma_k = (1 / pyr_scale^k - 1) / 2, s = max(round(5 sigma_k) | 1, 3)
 *   taps, BORDER_REFLECT_101) and resized INTER_LINEAR to round(H pyr_scale^k) x round(W pyr_scale^k); the polynomial expansion
 *   (poly_n, poly_sigma); the starting flow (zero, or the coarser level's resized and divided by pyr_scale); `iterations` times the
 *   (winsize / 2 * 2 + 1)^2 window sum of the matrices in float64, scaled by 1 / winsize^2, and the regularised 2 x 2 solve.
 *   tests/_farneback_ref.py restates every step in numpy.
 * No atomics and no host synchronisation: a pair's bits do not depend on B or on the run.
 *
 * in_dtype: EBOS_FARNEBACK_U8 / _F32 / _F64, the element type of prev and next (element strides prev_sb, prev_sr, next_sb,
 * next_sr; unit columns).  prev_sb = 0 shares one prev frame among all pairs (it is then expanded once).  out: device float32, the
 * flow (dx = column displacement, dy = row displacement) of pair b at row y, column x is out[b sb + y sr + x sx] = dx and
 * out[b sb + sc + y sr + x sx] = dy (element strides; [H, W, 2] and [2, H, W] layouts, or a view inside a larger frame).
 * pyr_scale in (0, 1), levels >= 0, winsize >= 1, iterations >= 1, poly_n 5 or 7, H, W >= 2, H * W < 2^31, B < 65535, else
 * EBOS_ERR_INVALID_ARG; flags other than 0 (OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_FARNEBACK_GAUSSIAN) are EBOS_ERR_UNSUPPORTED.
 * scratch: ebos_farneback_scratch_bytes(B, H, W, prev_sb == 0) bytes, 16-byte aligned (caller-owned); a short scratch is
 * EBOS_ERR_SCRATCH.  4 + iterations launches per level on `stream`.
 * ---------------------------------------------------------------------------------------- */
typedef enum ebos_farneback_dtype {
  EBOS_FARNEBACK_U8 = 0,
  EBOS_FARNEBACK_F32 = 1,
  EBOS_FARNEBACK_F64 = 2
} ebos_farneback_dtype;

size_t ebos_farneback_scratch_bytes(int B, int H, int W, int prev_shared);
int ebos_farneback(int in_dtype, int B, int H, int W, const void* prev, int64_t prev_sb, int64_t prev_sr, const void* next,
                   int64_t next_sb, int64_t next_sr, double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                   double poly_sigma, int flags, float* out, int64_t out_sb, int64_t out_sc, int64_t out_sr, int64_t out_sx,
                   void* scratch, size_t scratch_bytes, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Generative BOS solver (src/solver/patch_eklt_pyramid2.py, the reference YAML's patch_eklt_pyramid2), float64.
 *
 * ebos_gml_prepare_f64: per window, from the model image frame [H, W] (log(frame + 1) if use_log) and the polarity IWE
 *   pol [2, H, W]: gx, gy = cv2.Sobel(f, CV_64F, 0, 1 | 1, 0, ksize=3) (reflect-101); hist = pol0 -+ pol1 (+ if no_polarity);
 *   q = GaussianBlur(hist) with blur_taps (NULL: no blur), times we = GaussianBlur(|hist|) with weight_taps (both or neither
 *   of weight_taps / we), divided by its Frobenius norm; winv = 1 - 0.95 clip(g, 0, mean + std / 2) / max with
 *   g = scipy gaussian_filter(|hist|) with inv_taps (NULL: winv = 1).  Taps are device doubles [2 radius + 1].
 * ebos_gml_normalize_f64: q /= |q| (the reference divides its cached histogram in place once per scale).
 * ebos_gml_objective_f64: the objective at x [n_dim, gh, gw] (n_dim 3 = potential, p_x, p_y; 1 = potential) for patch
 *   = slide = `patch`: parts[4] = (loss, diff_norm, image_gradient, flow_norm_pxy) and grad = d loss / d x.
 * ebos_gml_solve_scale_f64: `iters` Adam steps (lr, betas 0.9 / 0.999, eps 1e-8, fresh state) on x in place; history
 *   (nullable) [iters, 4] as parts before each step; flow_out (nullable) [2, H, W] = the final F * M.
 * weights[3] = (w_diff_norm, w_image_gradient, w_flow_norm_pxy), 0 = absent; order[n_terms] = term indices (0, 1, 2) in the
 * configuration's order (the loss sums them in that order).  ROI rows [xmin, xmax), columns [ymin, ymax).  flags:
 * EBOS_GML_NO_POLARITY, EBOS_GML_EVENT_WEIGHTS (we is then required).  scratch: ebos_gml_scratch_bytes(H, W, smallest patch).
 * No atomics: results are bit-identical from run to run.  H, W >= 3, patch a power of two, else EBOS_ERR_INVALID_ARG.
 * ---------------------------------------------------------------------------------------- */
#define EBOS_GML_NO_POLARITY 1
#define EBOS_GML_EVENT_WEIGHTS 2

size_t ebos_gml_scratch_bytes(int H, int W, int min_patch);
int ebos_gml_prepare_f64(int H, int W, const double* frame, int use_log, const double* pol, int no_polarity, const double* blur_taps,
                         int blur_radius, const double* weight_taps, int weight_radius, const double* inv_taps, int inv_radius,
                         double* gx, double* gy, double* q, double* we, double* winv, void* scratch, size_t scratch_bytes,
                         ebos_stream_t stream);
int ebos_gml_normalize_f64(int64_t n, double* q, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_gml_objective_f64(int H, int W, int patch, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags, const double* weights,
                           const int* order, int n_terms, const double* gx, const double* gy, const double* q, const double* we,
                           const double* winv, const double* x, double* parts, double* grad, void* scratch, size_t scratch_bytes,
                           ebos_stream_t stream);
int ebos_gml_solve_scale_f64(int H, int W, int patch, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags, const double* weights,
                             const int* order, int n_terms, const double* gx, const double* gy, const double* q, const double* we,
                             const double* winv, double* x, int iters, double lr, double* history, double* flow_out, void* scratch,
                             size_t scratch_bytes, ebos_stream_t stream);

/* The window axis: n_windows (1 .. 65535) independent windows per call, one launch of every pass for all of them (the window is
 * the grid's z extent).  Window b is computed by exactly the operations, in the order, of the single-window entry, which is the
 * n_windows = 1 case of the same kernels: results are bit-identical to n_windows single calls.  Everything that differs per
 * window is window-major and contiguous: pol [B, 2, H, W]; gx, gy, q, we, winv [B, H, W]; x [B, n_dim, gh, gw]; flow_out
 * [B, 2, H, W]; history rows of window b at history + b * history_stride doubles (>= 4 iters).  frame_stride / grad_stride
 * (elements between windows) is H W, or 0 for one model image shared by all windows (gx, gy are then [H, W], formed once).
 * Geometry, cost weights, flags and iters are shared.  Scratch: ebos_gml_scratch_bytes_batch = n_windows slices of
 * ebos_gml_scratch_bytes; the solve entries use slice b at scratch + b * scratch_stride bytes (a multiple of 256, at least one
 * window's bytes); prepare and normalize lay their work planes out over the whole allocation. */
size_t ebos_gml_scratch_bytes_batch(int H, int W, int min_patch, int n_windows);
int ebos_gml_prepare_batch_f64(int n_windows, int H, int W, const double* frame, int64_t frame_stride, int use_log, const double* pol,
                               int no_polarity, const double* blur_taps, int blur_radius, const double* weight_taps, int weight_radius,
                               const double* inv_taps, int inv_radius, double* gx, double* gy, double* q, double* we, double* winv,
                               void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_gml_normalize_batch_f64(int n_windows, int64_t n, double* q, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_gml_solve_scale_batch_f64(int n_windows, int H, int W, int patch, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags,
                                   const double* weights, const int* order, int n_terms, const double* gx, const double* gy,
                                   int64_t grad_stride, const double* q, const double* we, const double* winv, double* x, int iters,
                                   double lr, double* history, int64_t history_stride, double* flow_out, void* scratch,
                                   size_t scratch_stride, size_t scratch_bytes, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Generative BOS solver, single scale (src/solver/patch_eklt_dependent.py, patch_eklt_dependent), float64.
 *
 * The grid: patch `patch`, slide `slide`, len(arange(0, L - patch + slide, slide)) cells per axis; pad k = patch / (2 slide) + 1
 * cells; the upsample is bilinear to (g + 2k) slide, centre-cropped (EBOS_ERR_INVALID_ARG where that crop leaves the canvas).
 * ebos_gml_dep_scratch_bytes: scratch of every entry below and of ebos_gml_prepare_f64 (canvas 0 x 0 without thresholding);
 *   0 for an invalid geometry.
 * ebos_gml_dep_select: sel [gh, gw] int32 = 1 + the cell's rank among the selected cells in row-major order, 0 = unselected;
 *   count[0] = the number selected.  row_box [gh, 3] / col_box [gw, 3] (device int32): the cell's event box [start, end) along
 *   the axis and whether its centre lies in the ROI (bounds inclusive).  With `thresholding` a cell must also hold more than
 *   event_thres of the events [n, 4] (x = row, y = column, ...), binned by floor into a canvas_h x canvas_w count image.
 * ebos_gml_dep_init_f64: x [n_dim, gh, gw] = 0, then x[0] = draws[rank] on the selected cells (draws NULL: all zero).
 * ebos_gml_dep_objective_f64 / ebos_gml_dep_solve_f64: as ebos_gml_objective_f64 / ebos_gml_solve_scale_f64, with the objective
 *   on the ROI crop [xmin, xmax) x [ymin, ymax) of the full-image gx, gy, q, we, winv (q is cropped and divided by the crop's
 *   norm), the gradient of unselected cells zero, and flow_out [2, H, W] the unmasked flow over the full image.  n_dim 1 / 3:
 *   Poisson model (F = up(Sobel3(x0) / 8)); with EBOS_GML_VELOCITY n_dim 2 / 4 (F = up(x[0:2])).  p_x, p_y = x[-2:].
 * ---------------------------------------------------------------------------------------- */
#define EBOS_GML_VELOCITY 4

size_t ebos_gml_dep_scratch_bytes(int H, int W, int patch, int slide, int xmin, int xmax, int ymin, int ymax, int canvas_h, int canvas_w);
int ebos_gml_dep_select(int H, int W, int patch, int slide, const int* row_box, const int* col_box, const double* events, int64_t n_events,
                        int canvas_h, int canvas_w, int thresholding, double event_thres, int* sel, int* count, void* scratch,
                        size_t scratch_bytes, ebos_stream_t stream);
int ebos_gml_dep_init_f64(int gh, int gw, int n_dim, const int* sel, const double* draws, double* x, ebos_stream_t stream);
int ebos_gml_dep_objective_f64(int H, int W, int patch, int slide, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags,
                               const double* weights, const int* order, int n_terms, const double* gx, const double* gy, const double* q,
                               const double* we, const double* winv, const int* sel, const double* x, double* parts, double* grad,
                               void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_gml_dep_solve_f64(int H, int W, int patch, int slide, int n_dim, int xmin, int xmax, int ymin, int ymax, int flags,
                           const double* weights, const int* order, int n_terms, const double* gx, const double* gy, const double* q,
                           const double* we, const double* winv, const int* sel, double* x, int iters, double lr, double* history,
                           double* flow_out, void* scratch, size_t scratch_bytes, ebos_stream_t stream);

/* The window axis of the single-scale solver (see above; the same kernels, n_windows = 1 being the entries above).  sel
 * [B, gh, gw], count [B] (read back once per batch), draws [B, gh gw] (window b uses its first count[b] values; NULL: all zero),
 * x [B, n_dim, gh, gw].  The events of all windows are one concatenated [n, 4] array; event_offsets [B + 1] (device int64) bound
 * each window's rows and max_events is the largest window's count.  Scratch: ebos_gml_dep_scratch_bytes_batch = n_windows slices
 * of ebos_gml_dep_scratch_bytes, slice b at scratch + b * scratch_stride bytes. */
size_t ebos_gml_dep_scratch_bytes_batch(int H, int W, int patch, int slide, int xmin, int xmax, int ymin, int ymax, int canvas_h,
                                        int canvas_w, int n_windows);
int ebos_gml_dep_select_batch(int n_windows, int H, int W, int patch, int slide, const int* row_box, const int* col_box,
                              const double* events, const int64_t* event_offsets, int64_t max_events, int canvas_h, int canvas_w,
                              int thresholding, double event_thres, int* sel, int* count, void* scratch, size_t scratch_stride,
                              size_t scratch_bytes, ebos_stream_t stream);
int ebos_gml_dep_init_batch_f64(int n_windows, int gh, int gw, int n_dim, const int* sel, const double* draws, double* x,
                                ebos_stream_t stream);
int ebos_gml_dep_solve_batch_f64(int n_windows, int H, int W, int patch, int slide, int n_dim, int xmin, int xmax, int ymin, int ymax,
                                 int flags, const double* weights, const int* order, int n_terms, const double* gx, const double* gy,
                                 int64_t grad_stride, const double* q, const double* we, const double* winv, const int* sel, double* x,
                                 int iters, double lr, double* history, int64_t history_stride, double* flow_out, void* scratch,
                                 size_t scratch_stride, size_t scratch_bytes, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * The sampled EKLT solvers, patch_eklt and generative_max_likelihood (src/solver/patch_eklt.py:101-136,
 * generative_max_likelihood.py:489-529), as a sweep in float64 (csrc/eklt_sweep.hip): every box is scored under every hypothesis
 *   P0 = v_x T_p(gx) + v_y T_p(gy) on the box (|P0| with EBOS_GML_NO_POLARITY, * we[box] with EBOS_GML_EVENT_WEIGHTS),
 *   P = P0 / (|P0|_F + 1e-4),  Q = q[box] / |q[box]|_F,  cost = w_diff_norm max_c sum_r |P - Q|,
 * T_p = cv2.warpPerspective of the whole image by the translation (p_x rows, p_y columns), INTER_LINEAR, BORDER_CONSTANT 0, in the
 * classic path: the source coordinate rounded to 1/32 pixel (half to even), the four float32 table weights, the sum in double.
 * gx, gy, q, we: the planes of ebos_gml_prepare_batch_f64 ([B, H, W]; gx, gy with grad_stride 0 = one model image; q holds the
 * event weights already, and any positive scale of it gives the same Q).
 * boxes [P, 4] (device int32): rows [r0, r1), columns [c0, c1), each inside the image and at most ph x pw; sel [B, P] (device
 * int32, NULL = all): 0 = do not evaluate.  A box that breaks these bounds, or whose |q[box]|_F is 0 or NaN, is not evaluated.
 * hyp [K, 4] (HOST float64): v_x, v_y, p_x, p_y per hypothesis; the entry derives the integer shift and the table weights once per
 * call.  cost [B, P, K] (NULL: not stored): written for every evaluated box, untouched elsewhere.  best_cost / best_index [B, P]:
 * the row minimum, the lowest index on a tie; a NaN cost never wins; +inf / -1 where no hypothesis won or the box is not
 * evaluated.  No atomics; a cost depends on its box and hypothesis alone, so results are bit-reproducible and do not depend on
 * the window's place in a batch or on how a table is cut into calls.
 * Routes: EBOS_EKLT_ROUTE_PATCH holds a box with a halo of ebos_eklt_sweep_halo(hyp, K) = max |integer shift| + 1 pixels in LDS --
 * 8 B x (2 (ph + 2 halo)(pw + 2 halo) + 2 ph pw) <= 160 KiB - 4 KiB, which ebos_eklt_sweep_fits reports -- and evaluates one
 * hypothesis per thread; EBOS_EKLT_ROUTE_ROI reads global memory with one workgroup per (hypothesis, box) (at most 65535 boxes),
 * for boxes up to the full image; EBOS_EKLT_ROUTE_AUTO takes the patch route where it fits.  The two routes sum in different
 * orders.  Scratch: ebos_eklt_sweep_scratch_bytes (route AUTO: enough for either).
 * ebos_eklt_patch_flow_batch_f64: grid [B, 2, gh, gw] = the winner's (v_x, v_y) of hyp [K, 4] (DEVICE float64; 0 where best_index
 * is -1), and flow [B, 2, H, W] = interpolate_dense_flow_from_patch_numpy of it (patch_eklt.py:138-171: edge pad
 * int(patch / 2 // slide) + 1 cells, bilinear x slide with half-pixel centres, centre crop).
 * ---------------------------------------------------------------------------------------- */
#define EBOS_EKLT_ROUTE_AUTO 0
#define EBOS_EKLT_ROUTE_PATCH 1
#define EBOS_EKLT_ROUTE_ROI 2

int ebos_eklt_sweep_fits(int ph, int pw, int halo);
int ebos_eklt_sweep_halo(const double* hyp, int n_hyp);
size_t ebos_eklt_sweep_scratch_bytes(int n_windows, int n_boxes, int n_hyp, int route);
int ebos_eklt_sweep_batch_f64(int n_windows, int H, int W, const double* gx, const double* gy, int64_t grad_stride, const double* q,
                              const double* we, const int* boxes, int n_boxes, int ph, int pw, const int* sel, const double* hyp,
                              int n_hyp, int flags, double w_diff_norm, int route, double* cost, double* best_cost, int* best_index,
                              void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_eklt_patch_flow_batch_f64(int n_windows, int H, int W, int patch, int slide, int gh, int gw, const int* best_index,
                                   const double* hyp, int n_hyp, double* grid, double* flow, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Perspective warp of camera frames into the event view: cv2.warpPerspective(src, M, (W, H), flags, BORDER_CONSTANT, border_value)
 * as the reference's co-capture loader applies it to every frame (src/data_loader/ccs.py:373-396), for B frames in one launch,
 * with the driver's validate_image crop (bos_event.py:25-39) fused in.  The arithmetic is OpenCV's classic fixed-point path
 * (4.5 - 4.10) as tests/_warp_ref.py restates it: M inverted in double on the host unless EBOS_WARP_INVERSE_MAP (closed-form
 * cofactors, one reciprocal); per pixel the double coordinates from the origin column of its block, 32 / W, round half to even,
 * 5 fraction bits (the clamp is fmin / fmax: a NaN coordinate, inf * 0 where 32 / W overflows, becomes INT_MAX, outside every
 * source); uint8: 15-bit weights, (sum + 16384) >> 15; float32: float weights, accumulated left to right; a tap outside
 * the source is border_value (uint8: rounded and saturated).  It restates that algorithm and is not checked against OpenCV.
 * No atomics, no scratch, no host synchronisation: a frame's bits do not depend on B, a pixel's bits not on the rectangle.
 *
 * dtype: EBOS_WARP_U8 / _F32, the element type of src and out.  src: device [B, Hs, Ws] (element strides src_sb, src_sr; unit
 * columns).  M: HOST doubles, one row-major 3 x 3 shared by the batch (m_stride 0) or one per frame (m_stride 9; then 32 frames
 * per launch); they travel as launch arguments, 72 bytes in the shared case.  Destination H rows x W columns; only rows
 * [xmin, xmax) and columns [ymin, ymax) (the reference's common_params names) are computed: pixel (row y, column x) of frame b
 * goes to out[b out_sb + (y - xmin) out_sr + (x - ymin)].
 * flags: EBOS_WARP_INTER_NEAREST or EBOS_WARP_INTER_LINEAR, optionally | EBOS_WARP_INVERSE_MAP; anything else is
 * EBOS_ERR_UNSUPPORTED.  Bad sizes (Hs, Ws <= 32767; H, W <= 65535), strides, rectangle, a non-finite border value, a matrix that
 * is singular, not finite or beyond 1e100 in magnitude: EBOS_ERR_INVALID_ARG, before anything is launched.
 * ---------------------------------------------------------------------------------------- */
typedef enum ebos_warp_dtype {
  EBOS_WARP_U8 = 0,
  EBOS_WARP_F32 = 1
} ebos_warp_dtype;
#define EBOS_WARP_INTER_NEAREST 0
#define EBOS_WARP_INTER_LINEAR 1
#define EBOS_WARP_INVERSE_MAP 16

int ebos_warp_perspective(int dtype, int B, int Hs, int Ws, const void* src, int64_t src_sb, int64_t src_sr, const double* M,
                          int64_t m_stride, int H, int W, int flags, double border_value, int xmin, int xmax, int ymin, int ymax,
                          void* out, int64_t out_sb, int64_t out_sr, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Lens calibration (csrc/rectify.hip): from a camera matrix K and OpenCV-order distortion coefficients D to rectified sub-pixel
 * events and rectified frames (reference: src/utils/event_utils.py:242-266 undistort_events, the loaders' load_calib / undistort,
 * src/solver/base.py:363-378 undistort_image).  tests/_rectify_ref.py restates every kernel in numpy with the same operation order.
 *
 * camera: 16 HOST doubles (fx, fy, cx, cy of K; fx', fy', cx', cy' of new_K; k1, k2, p1, p2, k3, k4, k5, k6), all finite, focal
 * lengths non-zero.  cx / fx belong to the column axis (sensor x), cy / fy to the row axis.  Forward model, ideal normalised (x, y)
 * -> sensor pixel (u, v), every operation rounded on its own:
 *   r2 = x x + y y;  rad = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2);  a = (2 x) y
 *   dx = p1 a + p2 (r2 + 2 (x x));  dy = p1 (r2 + 2 (y y)) + p2 a;  u = fx (x rad + dx) + cx;  v = fy (y rad + dy) + cy
 *
 *   ebos_rectify_map_f64      map [H, W, 2] float64 (16-byte aligned) = the rectified (row', col') of every sensor pixel: from
 *                             x0 = (col - cx) / fx, y0 = (row - cy) / fy exactly `iterations` (1 .. 1000) steps
 *                             x = (x0 - dx(x, y)) / rad(x, y), y = (y0 - dy(x, y)) / rad(x, y) starting at (x0, y0), then
 *                             (fy' y + cy', fx' x + cx').  One thread per pixel, plain stores.
 *   ebos_rectify_events_raw   raw columns (col / row int16, t int32 or int64 ticks, pol uint8) + that map -> events_out [m, 4] =
 *                             (row', col', ticks / ticks_per_second, pol != 0) float64 or float32 (out_is_f32), in stream order.
 *                             Dropped: an event whose pixel is outside the H x W sensor (the map is not read for it; counted in
 *                             counts[1]), and one whose rectified position, in the output's type, is not inside 0 <= row' < H_out,
 *                             0 <= col' < W_out.  counts: device int32 [2] = (m, dropped outside the sensor); the second kind of
 *                             drop is n - m - counts[1].  events_out holds n rows (16-byte aligned); rows past m are not written.
 *   ebos_undistort_events_*   the reference's undistort_events on events [n, 4]: k = int32(map_y[int32(x), int32(y)]),
 *                             l = int32(map_x[..]) (truncation toward zero; negative indices count from the end, as numpy's),
 *                             columns 0 and 1 replaced by k and l, rows with 0 <= k < h and 0 <= l < w kept in order.  map_x /
 *                             map_y: float64 [map_h, map_w].  counts: device int32 [2] = (m, events whose index numpy refuses).
 *   ebos_undistort_image_*    B frames [Hs, Ws] (uint8 or float32) rectified in one launch: output pixel (row r, column c) takes its
 *                             ideal position (c, r) -- M^-1 (c, r, 1) where M (HOST, 3 x 3, frame -> destination, may be NULL) is
 *                             given: the perspective kernel's coordinate walk --, normalises it by new_K, applies the forward model
 *                             and samples the source at (u, v) as ebos_warp_perspective's INTER_LINEAR does (rint(32 u), 5 fraction
 *                             bits, 15-bit weights or float products, constant border).  Where every coefficient is zero and new_K
 *                             equals K the lens step is skipped and the result is ebos_warp_perspective's bit for bit.  Rectangle,
 *                             strides and limits as there.
 * Events compact through a keep flag, the device-wide exclusive scan the plan build and ebos_filter_compact use, and a scatter;
 * scratch: ebos_rectify_scratch_bytes(n) bytes; n <= EBOS_RECTIFY_MAX_EVENTS.  No host synchronisation.
 * ---------------------------------------------------------------------------------------- */
#define EBOS_RECTIFY_MAX_EVENTS 2147000000LL

int ebos_rectify_map_f64(const double* camera, int iterations, int H, int W, double* map, ebos_stream_t stream);
size_t ebos_rectify_scratch_bytes(int64_t n);
int ebos_rectify_events_raw(const int16_t* col, const int16_t* row, const void* t, int t_is_int64, const uint8_t* pol, int64_t n,
                            double ticks_per_second, const double* map, int H, int W, int H_out, int W_out, int out_is_f32,
                            void* events_out, int32_t* counts, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_undistort_events_f32(const float* events, int64_t n, const double* map_x, const double* map_y, int map_h, int map_w, int h, int w,
                              float* events_out, int32_t* counts, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_undistort_events_f64(const double* events, int64_t n, const double* map_x, const double* map_y, int map_h, int map_w, int h, int w,
                              double* events_out, int32_t* counts, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_undistort_image_u8(int B, int Hs, int Ws, const uint8_t* src, int64_t src_sb, int64_t src_sr, const double* camera,
                            const double* M, int H, int W, double border_value, int xmin, int xmax, int ymin, int ymax, uint8_t* out,
                            int64_t out_sb, int64_t out_sr, ebos_stream_t stream);
int ebos_undistort_image_f32(int B, int Hs, int Ws, const float* src, int64_t src_sb, int64_t src_sr, const double* camera, const double* M,
                             int H, int W, double border_value, int xmin, int xmax, int ymin, int ymax, float* out, int64_t out_sb,
                             int64_t out_sr, ebos_stream_t stream);

/* ---- several solver windows' event side in one launch, from the raw sensor columns (csrc/window_ingest.hip) -----------------
 * col / row int16, t int32 (t_is_64 = 0) or int64 ticks, pol uint8: device columns of n_total events (RawEventStore.load_raw).
 * ranges: device int64 [B, 2], window b = events [begin, end) of the columns; ranges may overlap or be empty and are clamped to
 * [0, n_total]; max_len: an upper bound of end - begin known on the host (it only sizes the grid).  An event is kept when it lies
 * inside the CROP rectangle (has_roi: rows [xmin, xmax), columns [ymin, ymax), the solver's filter parameters) and outside the
 * removal rectangle (has_remove: rows [rm_x0, rm_x1), columns [rm_y0, rm_y1)).  Outputs, all overwritten:
 *   pol_out   double [B, 2, H, W]  events per pixel with p != 0 (channel 0) and p == 0 (channel 1): the float64 polarity image
 *                                  of the kept events (EBOS_SPLAT_POLARITY on integer pixels, whose weights are 1, 0, 0, 0);
 *   mask_out  uint8  [B, H, W]     1 where a kept event fell;
 *   count_out int64  [B]           kept events;  tmin_out / tmax_out double [B]: their first / last time, ticks /
 *                                  ticks_per_second in float64 (0 for a window that keeps nothing).
 * Counts are integers (LDS, then integer atomics); no floating-point atomic: every run gives the same bits.
 * scratch: ebos_window_ingest_scratch_bytes(B, H, W, has_roi, xmin, xmax, ymin, ymax) bytes, 256-byte aligned.  Two launches.
 * B <= 65535, H * W < 2^31 - 1, else EBOS_ERR_INVALID_ARG.
 * ---------------------------------------------------------------------------------------- */
size_t ebos_window_ingest_scratch_bytes(int B, int H, int W, int has_roi, int xmin, int xmax, int ymin, int ymax);
int ebos_window_ingest_raw_batch(const int16_t* col, const int16_t* row, const void* t, int t_is_64, const uint8_t* pol,
                                 int64_t n_total, double ticks_per_second, const int64_t* ranges, int B, int64_t max_len, int H,
                                 int W, int has_roi, int xmin, int xmax, int ymin, int ymax, int has_remove, int rm_x0, int rm_x1,
                                 int rm_y0, int rm_y1, double* pol_out, uint8_t* mask_out, int64_t* count_out, double* tmin_out,
                                 double* tmax_out, void* scratch, size_t scratch_bytes, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * The visualizer's pictures for B windows per launch (csrc/visualize.hip; reference: src/visualizer.py, src/solver/base.py:154-287).
 * Every plane is a device array of H W contiguous doubles (uint8 for masks) per window; window b of a plane starts sb elements
 * (mask_sb bytes) after window b - 1, so the two components of a [B, 2, H, W] flow are x = flow, y = flow + H W, sb = 2 H W.
 * Outputs are contiguous.  B <= 65535.  No floating-point atomics, no scratch: every run gives the same bits, and a window's
 * bits do not depend on the batch it is in.  The 8-bit HSV -> RGB step restates OpenCV's cvtColor(COLOR_HSV2RGB) on uint8
 * (hue 0 - 180, float32 sector arithmetic, round half to even) as tests/_viz_ref.py does; it is not checked against OpenCV.
 *
 * ebos_viz_reduce_f64: out[b, k] (device double [B, n_fields], overwritten) = the scalar field k's picture is normalised by.
 *   EBOS_VIZ_FLOW       max over pixels of sqrt(x^2 + y^2)^ord, NaN and +-inf components counted as 0; with a mask both
 *                       components are multiplied by (mask != 0) first (max_color_on_mask).
 *   EBOS_VIZ_FLOW_PAIR  the larger of that for (x, y) and for (x2, y2): the shared scale of visualize_optical_flow_pred_and_gt.
 *   EBOS_VIZ_SCALAR     max |x| (standardize_image_center); NaN entries are passed over.
 *   ord 0.5 is sqrt(sqrt(.)), ord 1 is sqrt(.), anything else pow.  fields: a HOST array of 1 .. EBOS_VIZ_MAX_FIELDS
 *   descriptors (it travels as a launch argument).  One memset node and one launch.
 * ebos_viz_flow_rgb_u8: color_optical_flow.  H = uint8((atan2(y, x) + pi) 180 / pi / 2), S = 255, V = uint8(255 mag / scale[b
 *   scale_stride]), HSV -> RGB; out uint8 [B, H, W, 3].  The casts truncate (NaN -> 0).  scale <= 0 (an all-zero flow) gives
 *   black.  mask (or NULL) with mask_mode: EBOS_VIZ_MASK_MULTIPLY multiplies the flow by (mask != 0) before anything else;
 *   EBOS_VIZ_MASK_BLACK / _WHITE paints the pixels with mask == 0 (Image.composite of visualize_optical_flow_on_event_mask).
 * ebos_viz_hsv2rgb_u8: the colour stage alone on n interleaved uint8 HSV pixels -> n RGB pixels.
 * ebos_viz_mask_close_u8: cv2.morphologyEx(mask != 0, MORPH_CLOSE, 3 x 3 MORPH_CROSS) with the default border (outside pixels
 *   never win the dilation and never lose the erosion); out uint8 [B, H, W] of 0 / 1, not aliasing mask.
 * ebos_viz_gray_u8: out uint8 [B, H - 2 pad, W - 2 pad], the inside of the H x W planes.
 *   EBOS_VIZ_GRAY_EVENT   clip(20 (a - b) + max_scale, 0, 255): a, b the positive and negative event counts, max_scale the
 *                         background colour, 127 in the reference (visualize_event)
 *   EBOS_VIZ_GRAY_IWE     255 - uint8(clip(max_scale (a + b), 0, 255)), b may be NULL (create_clipped_image; pad = outer_padding)
 *   EBOS_VIZ_GRAY_CENTER  uint8(a / scale[b scale_stride] 127 + 128); scale <= 0 (an all-zero field) gives 128
 * ---------------------------------------------------------------------------------------- */
#define EBOS_VIZ_MAX_FIELDS 8
#define EBOS_VIZ_FLOW 0
#define EBOS_VIZ_FLOW_PAIR 1
#define EBOS_VIZ_SCALAR 2
#define EBOS_VIZ_MASK_MULTIPLY 1
#define EBOS_VIZ_MASK_BLACK 2
#define EBOS_VIZ_MASK_WHITE 4
#define EBOS_VIZ_GRAY_EVENT 0
#define EBOS_VIZ_GRAY_IWE 1
#define EBOS_VIZ_GRAY_CENTER 2

typedef struct ebos_viz_field {
  const double* x;       /* first component, or the scalar field */
  const double* y;
  const double* x2;      /* EBOS_VIZ_FLOW_PAIR: the second flow */
  const double* y2;
  const uint8_t* mask;   /* EBOS_VIZ_FLOW: optional */
  int64_t sb;            /* window stride of x, y (elements) */
  int64_t sb2;           /* ... of x2, y2 */
  int64_t mask_sb;
  int kind;
  int reserved;
} ebos_viz_field;

int ebos_viz_reduce_f64(int B, int H, int W, const ebos_viz_field* fields, int n_fields, double ord, double* out,
                        ebos_stream_t stream);
int ebos_viz_flow_rgb_u8(int B, int H, int W, const double* x, const double* y, int64_t sb, const double* scale,
                         int64_t scale_stride, const uint8_t* mask, int64_t mask_sb, int mask_mode, double ord, uint8_t* out,
                         ebos_stream_t stream);
int ebos_viz_hsv2rgb_u8(int64_t n, const uint8_t* hsv, uint8_t* rgb, ebos_stream_t stream);
int ebos_viz_mask_close_u8(int B, int H, int W, const uint8_t* mask, int64_t mask_sb, uint8_t* out, ebos_stream_t stream);
int ebos_viz_gray_u8(int mode, int B, int H, int W, int pad, const double* a, int64_t a_sb, const double* b, int64_t b_sb,
                     double max_scale, const double* scale, int64_t scale_stride, uint8_t* out, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Time-resolved event representations (csrc/event_voxel.hip; reference: src/utils/event_utils.py:291-440).  All buffers are device
 * memory, outputs are contiguous and overwritten.  Every addend of a voxel is the reference's addend bit for bit (no fused
 * multiply-add, the reference's order of operations); the order in which the float atomics add them is free.  Taps whose weight
 * is exactly zero are skipped.
 *
 * ebos_event_voxel_f64: create_event_voxel.  x (the width direction), y, pol, t: n doubles each; out double [C, H, W].
 *   t_norm = (C - 1) (t - t[0]) / (t[n - 1] - t[0]); x0, y0, t0 truncated towards zero; the eight corners {x0, x0 + 1} x {y0, y0 + 1}
 *   x {t0, t0 + 1} inside the grid get ((pol (1 - |xl - x|)) (1 - |yl - y|)) (1 - |tl - t_norm|).  status (device int): 1, or 0
 *   when t[n - 1] - t[0] is zero or not finite -- the grid is then all zero (the reference divides by zero there).  One memset
 *   node and one launch.
 * ebos_event_voxel_normalize_f64: B grids of n voxels each, in place: the non-zero voxels v become (v - mean) / std with their
 *   mean and unbiased std, v - mean when std is not > 0; a grid without a non-zero voxel is left alone.  scratch:
 *   ebos_event_voxel_normalize_scratch_bytes(B) bytes (the partial moments), 8-byte aligned.  One reduction launch, one map
 *   launch, nothing read back.
 * ebos_event_volume_f64 / _f32: generate_discretized_event_volume.  events [n, 4] = (x = row, y = column, t, p) contiguous;
 *   out [T, X, Y] in the events' type; nb = T / 2, t_scaled = (t - tmin) ((1 / (tmax - tmin)) (nb - 1)) (torch's tensor
 *   __rdiv__), tmin / tmax reduced on the device; bin floor(ts + 1e-8) gets floor(ts) + 1 - ts, bin ceil(ts - 1e-8) gets
 *   ts - floor(ts + 1e-8), + nb for p < 0, pixel x Y + y of the truncated coordinates.  status: device int64 [4]; status[0] holds
 *   the flags below afterwards (0: fine), status[1 .. 2] are the keys of the time range.  A vote outside the volume (what the
 *   reference asserts against) is not made and sets EBOS_EVENT_VOLUME_OUT_OF_BOUNDS; tmax == tmin leaves the volume zero and
 *   sets EBOS_EVENT_VOLUME_DEGENERATE_SPAN.  T >= 2.  Three memset nodes and two launches.
 * ebos_event_voxel_raw_batch: the voxel grids of B windows of a recording from its raw columns (col / row int16, t int32 or,
 *   t_is_64, int64 ticks, pol uint8: n_total events, RawEventStore.load_raw), x = col, y = row, t = ticks / ticks_per_second in
 *   float64, pol = +-1 (signed_pol) or 0 / 1.  ranges: device int64 [B, 2], window b = events [begin, end), clamped to
 *   [0, n_total]; they may overlap, be empty and come in any order; max_len: an upper bound of end - begin known on the host (it
 *   sizes the grid).  has_roi: only events in rows [xmin, xmax) x columns [ymin, ymax) are kept, the grid is the crop (H = xmax -
 *   xmin, W = ymax - ymin) and the coordinates are shifted by its origin -- crop_event first, then create_event_voxel.  A window's
 *   time bounds are those of its first and last kept event, read from the time-sorted column.  out double [B, C, H, W];
 *   valid int [B]: 0 and an all-zero grid for a window that keeps fewer than two events or spans no time; bounds int64 [B, 2]:
 *   the indices of the first and last kept event (-1, -1 where valid is 0).  One memset node and two launches, whatever B is.
 *   B <= 65535.
 * ---------------------------------------------------------------------------------------- */
#define EBOS_VOXEL_NORM_PARTIALS 256
#define EBOS_EVENT_VOLUME_OUT_OF_BOUNDS 1
#define EBOS_EVENT_VOLUME_DEGENERATE_SPAN 2

int ebos_event_voxel_f64(const double* x, const double* y, const double* pol, const double* t, int64_t n, int C, int H, int W,
                         double* out, int* status, ebos_stream_t stream);
size_t ebos_event_voxel_normalize_scratch_bytes(int B);
int ebos_event_voxel_normalize_f64(int B, int64_t n, double* grid, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_event_volume_f64(const double* events, int64_t n, int T, int X, int Y, double* out, int64_t* status, ebos_stream_t stream);
int ebos_event_volume_f32(const float* events, int64_t n, int T, int X, int Y, float* out, int64_t* status, ebos_stream_t stream);
int ebos_event_voxel_raw_batch(const int16_t* col, const int16_t* row, const void* t, int t_is_64, const uint8_t* pol, int64_t n_total,
                               double ticks_per_second, const int64_t* ranges, int B, int64_t max_len, int C, int H, int W,
                               int has_roi, int xmin, int xmax, int ymin, int ymax, int signed_pol, double* out, int* valid,
                               int64_t* bounds, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Time-aware flow (csrc/flow_voxel.hip; reference: src/utils/flow_utils.py:68-702): a dense flow at t0 becomes a flow per time
 * bin.  All buffers are device memory and contiguous, outputs are overwritten and never alias inputs.  flow[.., 0, :, :] moves
 * along the rows (H), flow[.., 1, :, :] along the columns.  Every operation is rounded on its own and in the reference's order
 * (no fused multiply-add): the advection kernels reproduce the reference bit for bit; NaN propagates as through np.maximum.
 *
 * ebos_flow_upwind_step_* / ebos_flow_burgers_step_*: one step of upwind_flow_to_voxel / inviscid_burger_flow_to_voxel on
 *   B flows [B, 2, H, W] -> out [B, 2, H, W].  dt != 0; a negative dt steps the negated flow and negates the result.  The upwind
 *   step divides u_dx and u_dy by dx and v_dx and v_dy by dy, the Burgers step u_dy by dx and v_dx by dy, as the reference does.
 *   One launch.  B <= 32767.
 * ebos_flow_voxel_advect_*: construct_dense_flow_voxel for scheme EBOS_FLOW_UPWIND / _BURGERS / _SAME: flow [B, 2, H, W] ->
 *   out [B, T, 2, H, W].  Bin t0_index is the input, bin t0_index - s is s steps with dt = -1 / T, bin t0_index + s is s steps
 *   with +1 / T (dx = dy = 1); _SAME copies the input into every bin.  has_clamp: every stored value is min(max(v, -clamp),
 *   clamp); the steps themselves run on unclamped values.  wrap_last (the reference's torch Burgers constructor, whose backward
 *   loop runs one step too far and stores it in bin -1): when t0_index == T - 1 the chain takes t0_index + 1 backward steps and
 *   the last one replaces bin T - 1; otherwise nothing changes, because the forward chain overwrites that bin.  route:
 *   EBOS_FLOW_ROUTE_AUTO takes one launch for the whole voxel (a 32 x 32 tile with its halo in LDS, all steps there) when
 *   neither direction needs more than ebos_flow_voxel_halo_cap() steps and one launch per step otherwise; _FUSED / _STEPS force
 *   either (_FUSED beyond the cap is an error).  The two routes store identical bits.
 * ebos_flow_voxel_propagate_bilinear_*: propagate_flow_to_voxel(.., "bilinear") for B flows and T time offsets: out [B, T, 2,
 *   H, W], bin t with dt = (t - t_offset) / denominator in double when denominator > 0, else dt (T = 1 then serves the
 *   stand-alone function).  Pixel (i, j) votes both flow components into cells (x1, y1), (x1 + 1, y1), (x1, y1 + 1), (x1 + 1,
 *   y1 + 1) of (x, y) = (i + u dt, j + v dt), x1 = floor(x + 1e-8), with the weights (1 - fx)(1 - fy), (1 - fx) fy, fx (1 - fy),
 *   fx fy in that order (the reference's order); a vote outside the image adds value * 0 to cell 0.  Float atomics: the addends
 *   are the reference's, their order is free.  One memset node, one launch, one more launch with a clamp.  B * T <= 65535.
 * ebos_flow_voxel_truncate_mean_*: truncate_voxel_flow(.., "mean"): voxel [T, 2, H, W] -> out double [2, H, W] =
 *   sum_t(flow * mask) / (sum_t(mask) + 1e-6), mask = (u u + v v > 0), the bins added in index order.  One launch.
 * ---------------------------------------------------------------------------------------- */
#define EBOS_FLOW_UPWIND 0
#define EBOS_FLOW_BURGERS 1
#define EBOS_FLOW_SAME 2
#define EBOS_FLOW_ROUTE_AUTO 0
#define EBOS_FLOW_ROUTE_FUSED 1
#define EBOS_FLOW_ROUTE_STEPS 2
#define EBOS_FLOW_VOXEL_HALO_CAP 8

int ebos_flow_voxel_halo_cap(void);
int ebos_flow_voxel_advect_f32(int scheme, int B, int T, int H, int W, const float* flow, float* out, int t0_index, int has_clamp,
                               double clamp, int wrap_last, int route, ebos_stream_t stream);
int ebos_flow_voxel_advect_f64(int scheme, int B, int T, int H, int W, const double* flow, double* out, int t0_index, int has_clamp,
                               double clamp, int wrap_last, int route, ebos_stream_t stream);
int ebos_flow_upwind_step_f32(int B, int H, int W, const float* flow, float* out, double dt, double dx, double dy, ebos_stream_t stream);
int ebos_flow_upwind_step_f64(int B, int H, int W, const double* flow, double* out, double dt, double dx, double dy, ebos_stream_t stream);
int ebos_flow_burgers_step_f32(int B, int H, int W, const float* flow, float* out, double dt, double dx, double dy, ebos_stream_t stream);
int ebos_flow_burgers_step_f64(int B, int H, int W, const double* flow, double* out, double dt, double dx, double dy, ebos_stream_t stream);
int ebos_flow_voxel_propagate_bilinear_f32(int B, int T, int H, int W, const float* flow, float* out, int t_offset, int denominator,
                                           double dt, int has_clamp, double clamp, ebos_stream_t stream);
int ebos_flow_voxel_propagate_bilinear_f64(int B, int T, int H, int W, const double* flow, double* out, int t_offset, int denominator,
                                           double dt, int has_clamp, double clamp, ebos_stream_t stream);
int ebos_flow_voxel_truncate_mean_f32(int T, int H, int W, const float* voxel, double* out, ebos_stream_t stream);
int ebos_flow_voxel_truncate_mean_f64(int T, int H, int W, const double* voxel, double* out, ebos_stream_t stream);

/* ---------------------------------------------------------------------------------------- *
 * Backward of the time-aware flow with respect to the flow at t0 (csrc/flow_voxel_grad.hip).  Every kernel gathers, in a fixed
 * order and without atomics: two runs give the same bits.  The derivative rules are torch's: maximum(x, 0) and minimum(x, 0) pass
 * half the gradient each where x == 0, sign() and floor() none; a clamp passes the gradient where -clamp <= x <= clamp.
 *
 * ebos_flow_upwind_step_adjoint_* / ebos_flow_burgers_step_adjoint_*: flow [B, 2, H, W] is the input of the step with (dt, dx, dy),
 *   grad_out the gradient of its output -> grad_in the gradient of its input.  One launch.
 * ebos_flow_voxel_advect_adjoint_*: the arguments of ebos_flow_voxel_advect_* with voxel [B, T, 2, H, W] = its UNCLAMPED output
 *   (not read for _SAME, may be NULL) and grad_voxel the gradient of the (clamped, if has_clamp) voxel -> grad_flow [B, 2, H, W].
 *   The bins are the intermediates of the chain; the walk goes from the outer bins towards t0 and adds each bin's upstream
 *   gradient as it passes.  Routes as in the forward: one launch with a tile (32 x 32 for float, 24 x 24 for double), its halo and the
 *   running gradient in LDS, or one launch per step through workspace, which holds
 *   ebos_flow_voxel_advect_adjoint_workspace(..) elements (0: not needed, may be NULL; -1: bad arguments).
 * ebos_flow_voxel_propagate_bilinear_adjoint_*: the arguments of ebos_flow_voxel_propagate_bilinear_* with voxel = its unclamped
 *   output (read with has_clamp only) and grad_voxel -> grad_flow: per source pixel the four weights times the gradient at its four
 *   cells plus the part through the position (d fx / d flow[0] = dt, d fy / d flow[1] = dt), summed over the bins in index order.
 * ebos_flow_voxel_clamp_*: out[i] = min(max(in[i], -clamp), clamp), NaN kept; out of place, for the clamped copy of a kept voxel.
 * ---------------------------------------------------------------------------------------- */
int64_t ebos_flow_voxel_advect_adjoint_workspace(int scheme, int B, int T, int H, int W, int t0_index, int wrap_last, int route);
int ebos_flow_upwind_step_adjoint_f32(int B, int H, int W, const float* flow, const float* grad_out, float* grad_in, double dt, double dx,
                                      double dy, ebos_stream_t stream);
int ebos_flow_upwind_step_adjoint_f64(int B, int H, int W, const double* flow, const double* grad_out, double* grad_in, double dt, double dx,
                                      double dy, ebos_stream_t stream);
int ebos_flow_burgers_step_adjoint_f32(int B, int H, int W, const float* flow, const float* grad_out, float* grad_in, double dt, double dx,
                                       double dy, ebos_stream_t stream);
int ebos_flow_burgers_step_adjoint_f64(int B, int H, int W, const double* flow, const double* grad_out, double* grad_in, double dt, double dx,
                                       double dy, ebos_stream_t stream);
int ebos_flow_voxel_advect_adjoint_f32(int scheme, int B, int T, int H, int W, const float* flow, const float* voxel, const float* grad_voxel,
                                       float* grad_flow, int t0_index, int has_clamp, double clamp, int wrap_last, int route, float* workspace,
                                       ebos_stream_t stream);
int ebos_flow_voxel_advect_adjoint_f64(int scheme, int B, int T, int H, int W, const double* flow, const double* voxel, const double* grad_voxel,
                                       double* grad_flow, int t0_index, int has_clamp, double clamp, int wrap_last, int route, double* workspace,
                                       ebos_stream_t stream);
int ebos_flow_voxel_propagate_bilinear_adjoint_f32(int B, int T, int H, int W, const float* flow, const float* voxel, const float* grad_voxel,
                                                   float* grad_flow, int t_offset, int denominator, double dt, int has_clamp, double clamp,
                                                   ebos_stream_t stream);
int ebos_flow_voxel_propagate_bilinear_adjoint_f64(int B, int T, int H, int W, const double* flow, const double* voxel, const double* grad_voxel,
                                                   double* grad_flow, int t_offset, int denominator, double dt, int has_clamp, double clamp,
                                                   ebos_stream_t stream);
int ebos_flow_voxel_clamp_f32(int64_t n, const float* in, float* out, double clamp, ebos_stream_t stream);
int ebos_flow_voxel_clamp_f64(int64_t n, const double* in, double* out, double clamp, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Time-aware warp: every event is displaced by the flow of ITS OWN time bin of a flow voxel
 *   (voxel [(b,) T, 2, H, W] as ebos_flow_voxel_advect_* / _propagate_bilinear_* write it, channel 0 = rows).
 *   The reference documents the motion model ("dense-flow-voxel-optimized", src/warp.py:199, 211) and
 *   ships without its branch (:223-228); this is A3 and the fused hot path with one more gather index.
 *
 * bin      tau = (t - tmin) / (tmax - tmin) evaluated in float64 whatever the event type (float32 times
 *          are widened exactly);  k = min((int)(tau * T), T - 1);  tmax == tmin -> k = 0 for every event.
 *          The bin does not depend on the reference time.  1 <= T <= 255 everywhere below.
 * warp     i = trunc(x) * row_stride + trunc(y)
 *          x' = x - dt * voxel[k][0][i];  y' = y - dt * voxel[k][1][i];  t' = dt;  p' = p
 *          dt, the operation order, the rounding (no FMA contraction), the out-of-range rule and
 *          *oob_count exactly as ebos_warp_dense_*.
 * Every entry reads a bin as min(bins[i], T - 1), so a bins array made for another T never indexes
 * outside the voxel.
 *
 * ebos_event_time_bins_*   events [b, n, 4], tminmax [b, 2] (ebos_time_range_*) -> bins [b, n] uint8.
 * ebos_warp_voxel_*        the arguments of ebos_warp_dense_* plus T and bins [b, n]; voxel [b, T, 2, H, W].
 * ebos_warp_voxel_bwd_*    d_voxel[k][c][i] += -dt * d_warped[..., c]  (accumulates; d_voxel [b, T, 2, H, W]).
 * ---------------------------------------------------------------------------------------- */
int ebos_event_time_bins_f32(const float* events, const float* tminmax, int64_t b, int64_t n, int T, uint8_t* bins,
                             ebos_stream_t stream);
int ebos_event_time_bins_f64(const double* events, const double* tminmax, int64_t b, int64_t n, int T, uint8_t* bins,
                             ebos_stream_t stream);
int ebos_warp_voxel_f32(const float* events, const float* voxel, const float* tminmax, int ref_mode, double ref_fraction,
                        int normalize_t, int64_t b, int64_t n, int T, int H, int W, int row_stride, const uint8_t* bins,
                        float* warped, int32_t* oob_count, ebos_stream_t stream);
int ebos_warp_voxel_f64(const double* events, const double* voxel, const double* tminmax, int ref_mode, double ref_fraction,
                        int normalize_t, int64_t b, int64_t n, int T, int H, int W, int row_stride, const uint8_t* bins,
                        double* warped, int32_t* oob_count, ebos_stream_t stream);
int ebos_warp_voxel_bwd_f32(const float* events, const float* tminmax, int ref_mode, double ref_fraction, int normalize_t,
                            const float* d_warped, int64_t b, int64_t n, int T, int H, int W, int row_stride,
                            const uint8_t* bins, float* d_voxel, ebos_stream_t stream);
int ebos_warp_voxel_bwd_f64(const double* events, const double* tminmax, int ref_mode, double ref_fraction, int normalize_t,
                            const double* d_warped, int64_t b, int64_t n, int T, int H, int W, int row_stride,
                            const uint8_t* bins, double* d_voxel, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused hot path of the time-aware warp: the three entries of the dense-flow path with the gather
 *   voxel[(k * 2 + c) * H * W + i] and the bins (uint8 [n], in the order of the events) as one more SoA stream.
 *   x, y, dt, weight(nullable): SoA f32 [n];  voxel [T, 2, H, W];  iwe [h, w] with h = H + 2 pad_h ...
 * ebos_iwe_voxel_f32        any event order; one global float atomic per tap.  Accumulates into iwe.
 * ebos_iwe_voxel_tiled_f32  binned events: ebos_iwe_dense_tiled_f32's organisation, (tile_h, tile_w, halo)
 *   configurations (ebos_tiled_config), LDS accumulator rule and spill path beyond the halo.  Accumulates into iwe.
 * ebos_iwe_voxel_bwd_f32    g_image / affine / g_lo / d_weight as in ebos_iwe_dense_bwd_f32;
 *   d_voxel[k][c][i] += -dt * dL/d(x', y')  (accumulates; d_voxel [T, 2, H, W]).  sorted != 0 promises that
 *   events sharing a source pixel are contiguous; the wave's segmented reduction keys on (k, i), so the
 *   result is right for any order of a pixel's events among its bins.
 * ---------------------------------------------------------------------------------------- */
int ebos_iwe_voxel_f32(const float* x, const float* y, const float* dt, const float* weight, const uint8_t* bins, int64_t n,
                       const float* voxel, int T, int H, int W, int row_stride, int pad_h, int pad_w, float* iwe,
                       ebos_stream_t stream);
int ebos_iwe_voxel_tiled_f32(const float* xs, const float* ys, const float* dts, const float* weight, const uint8_t* bins,
                             const int32_t* key_offsets, int64_t n, const float* voxel, int T, int H, int W, int tile_h,
                             int tile_w, int halo, int splits, int pad_h, int pad_w, float* iwe, ebos_stream_t stream);
int ebos_iwe_voxel_bwd_f32(const float* x, const float* y, const float* dt, const float* weight, const uint8_t* bins,
                           int64_t n, const float* voxel, int T, int H, int W, int row_stride, int pad_h, int pad_w,
                           const float* g_image, const float* affine, int g_lo, int sorted, float* d_voxel, float* d_weight,
                           ebos_stream_t stream);
/* ebos_iwe_voxel_owner_bwd_f32: the addends of ebos_iwe_voxel_bwd_f32 for a BINNED plan (xs / ys / dts / bins in key order and
 *   key_offsets of ebos_bin_events_f32 with (tile_h, tile_w)), summed by the owner of each source pixel: the lane that walks the
 *   pixel's run key_offsets[key] .. key_offsets[key + 1] is the only writer of its 2 T cells.  No atomics; d_voxel [T, 2, H, W] is
 *   OVERWRITTEN, every cell of it (zeros where no event lands, pixels of empty tiles included), so the caller neither clears nor
 *   zero-allocates it; the order of the additions is the plan's, so two calls give the same bits.  Runs of more than 64 events
 *   (a hot pixel) are walked by the whole wave with a fixed reduction tree per bin.  weight nullable; no d_weight. */
int ebos_iwe_voxel_owner_bwd_f32(const float* xs, const float* ys, const float* dts, const float* weight, const uint8_t* bins,
                                 const int32_t* key_offsets, int64_t n, const float* voxel, int T, int H, int W, int tile_h,
                                 int tile_w, int pad_h, int pad_w, const float* g_image, const float* affine, int g_lo,
                                 float* d_voxel, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-reference contrast: the IWEs of ONE dense flow at K <= EBOS_MULTIREF_MAX reference times from one pass over a binned plan.
 * A plan built with normalised time and reference fraction f holds dt = (t - tmin) / (tmax - tmin) - f; the dt of reference
 * fraction r is dt + (f - r), so reference k is the scalar shifts[k] = f - r_k (HOST memory, float [K], finite; it travels to the
 * kernels by value):   dt_k = dt + shifts[k] (float32);  x'_k = x - dt_k * flow[0][pix];  y'_k = y - dt_k * flow[1][pix].
 * An event is decoded once and its flow cell gathered once for all K references.  No per-event weights.
 *   xs, ys, dts: SoA f32 [n] in key order with key_offsets of ebos_bin_events_f32 (tile_h, tile_w);  flow [2, H, W].
 * ebos_iwe_multiref_fits (host only): how K LDS windows of tile + halo are kept -- 2: f64, 1: f32 (ebos_iwe_dense_tiled_f32's
 *   accumulator rule applied to K windows), 0: they do not fit the 160 KiB LDS, K is outside [1, EBOS_MULTIREF_MAX], or
 *   (tile_h, tile_w, halo) is no ebos_tiled_config.
 * ebos_iwe_dense_multiref_tiled_f32: ebos_iwe_dense_tiled_f32's organisation with K windows per (tile, split) workgroup; the votes,
 *   their eps and the spill path beyond the halo (global float atomics) are that kernel's.  iwes [K, h, w], h = H + 2 pad_h ...;
 *   ACCUMULATES into iwes.  EBOS_ERR_UNSUPPORTED, and no launch, where ebos_iwe_multiref_fits is 0.
 * ebos_iwe_dense_multiref_owner_bwd_f32: d_flow[c][i] = sum over the events of source pixel i and the references k of
 *   -dt_k * dL/d(x'_k, y'_k), the four taps read from G_k = a_k * g_images[k] + c_k (g_images [K, h, w]; affine [K, 2] on the device,
 *   nullable: a = 1, c = 0), G_k = 0 outside [g_lo, h - g_lo) x [g_lo, w - g_lo).  The pattern of ebos_iwe_voxel_owner_bwd_f32: the
 *   lane that walks a pixel's run gathers the flow cell once and is the only writer of the pixel's two cells.  No atomics;
 *   d_flow [2, H, W] is OVERWRITTEN, every cell of it (zeros where no event lies, pixels of empty tiles included); the order of the
 *   additions is the plan's, so two calls give the same bits.  Runs of more than 64 events (a hot pixel) are walked by the whole
 *   wave with a fixed reduction tree.
 * ---------------------------------------------------------------------------------------- */
#define EBOS_MULTIREF_MAX 4
int ebos_iwe_multiref_fits(int tile_h, int tile_w, int halo, int K);
int ebos_iwe_dense_multiref_tiled_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                      const float* flow, int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h,
                                      int pad_w, const float* shifts, int K, float* iwes, ebos_stream_t stream);
int ebos_iwe_dense_multiref_owner_bwd_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                          const float* flow, int H, int W, int tile_h, int tile_w, int pad_h, int pad_w,
                                          const float* shifts, int K, const float* g_images, const float* affine, int g_lo,
                                          float* d_flow, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Second order on the plain dense-flow warp: the tangent image of the IWE and the Hessian-vector product of a contrast that is
 * quadratic in the image (both shipped contrasts are), on a binned plan with its SoA events.  v [2, H, W] is the direction.
 * An event with source pixel s, flow cell flow[:, s] and taps / fractions (fr, fc) of its warped position moves, along v, by
 * (tx, ty) = (-dt v[0][s], -dt v[1][s]).
 * ebos_iwe_dense_tangent_tiled_f32: u = d IWE(flow + e v) / de at e = 0, the splat of ebos_iwe_dense_multiref_tiled_f32 with the
 *   four weights replaced by their derivatives along (tx, ty):
 *       w00' = -(1-fc) tx - (1-fr) ty     w10' = (1-fc) tx - fr ty     w01' = -fc tx + (1-fr) ty     w11' = fc tx + fr ty
 *   One LDS window per (tile, split) workgroup for u and, where iwe is not NULL, a second one for the IWE of the same pass; f64 windows
 *   where ebos_iwe_multiref_fits(tile_h, tile_w, halo, iwe ? 2 : 1) is 2, f32 where it is 1, EBOS_ERR_UNSUPPORTED and no launch where
 *   it is 0.  tangent and iwe are [h, w], h = H + 2 pad_h ...; the kernel ACCUMULATES into them (the caller zero-fills), beyond the
 *   halo with global float atomics.
 * ebos_iwe_dense_hvp_owner_bwd_f32: with G1 = a1 g1 + c1 and G2 = a2 g2 + c2 inside [g_lo, h - g_lo) x [g_lo, w - g_lo), 0 outside
 *   (g1 = the cost's gradient map at the IWE, g2 = the same map at u; affine = (a1, c1, a2, c2) on the device, nullable: a = 1, c = 0),
 *       dx(G) = (1-fc)(G10-G00) + fc(G11-G01)    dy(G) = (1-fr)(G01-G00) + fr(G11-G10)    cross = G1_00 - G1_10 - G1_01 + G1_11
 *       hv[:, s]     = sum over the events of s of -dt (dx(G2) + cross ty,  dy(G2) + cross tx)
 *       d_flow[:, s] = sum over the events of s of -dt (dx(G1), dy(G1))                               (nullable: not written)
 *   The pattern of ebos_iwe_dense_multiref_owner_bwd_f32: the lane that walks a pixel's run is the only writer of its cells.  No
 *   atomics; hv (and d_flow) [2, H, W] are OVERWRITTEN, every cell (zeros where no event lies, n == 0 included); the order of the
 *   additions is the plan's, so two calls give the same bits.  Runs of more than 64 events are walked by the whole wave with a fixed
 *   reduction tree.
 * ebos_iwe_dense_tangent_slab_f32: the same images with bits that repeat.  The tangent kernel's sums over the windows of neighbouring
 *   tiles meet in global float atomics, whose order the hardware picks: where three or more windows overlap, the last bits differ
 *   from call to call.  Here every tile (one work item per tile) stores its window(s) to its slab of `workspace`
 *   (ebos_iwe_tangent_slab_workspace_bytes, host only: 0 where ebos_iwe_multiref_fits is 0; no zero-fill needed) and a combine pass
 *   adds to every image cell the slabs that cover it, in tile order, summed in f64.  Same arguments otherwise, same convention (the
 *   caller zero-fills the images), same spill path beyond the halo -- the one part that stays atomic.  EBOS_ERR_SCRATCH for a
 *   workspace that is too small.  The bits repeat where the windows are f64 and nothing spills.
 * All three refuse NULL buffers and bad sizes (EBOS_ERR_INVALID_ARG) before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int ebos_iwe_dense_tangent_tiled_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                     const float* flow, const float* v, int H, int W, int tile_h, int tile_w, int halo, int splits,
                                     int pad_h, int pad_w, float* iwe, float* tangent, ebos_stream_t stream);
size_t ebos_iwe_tangent_slab_workspace_bytes(int H, int W, int tile_h, int tile_w, int halo, int windows);
int ebos_iwe_dense_tangent_slab_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                    const float* flow, const float* v, int H, int W, int tile_h, int tile_w, int halo, int pad_h,
                                    int pad_w, void* workspace, size_t workspace_bytes, float* iwe, float* tangent,
                                    ebos_stream_t stream);
int ebos_iwe_dense_hvp_owner_bwd_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                     const float* flow, const float* v, int H, int W, int tile_h, int tile_w, int pad_h, int pad_w,
                                     const float* g1, const float* g2, const float* affine, int g_lo, float* d_flow, float* hv,
                                     ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-reference contrast on the tile-private pipeline: the K-image form of ebos_iwe_dense_slab_f32 / ebos_iwe_dense_tiled_bwd_f32.
 * Events, shifts and K as above: dt_k = dt + shifts[k] is ONE rounded float32 add per event, before anything else uses it.
 * ebos_slab_multiref_config (host only): the built (tile_h, tile_w, halo) triples, as ebos_slab_config lists the single form's.
 * ebos_iwe_slab_multiref_workspace_bytes (host only): K workspaces of the single form back to back (0: bad arguments, K outside
 *   [1, EBOS_MULTIREF_MAX], splits < 1 or an unbuilt triple).  ZERO-FILLED ONCE by the caller; the spill / SpillEpoch / counter
 *   contract of every one of the K sections is ebos_iwe_dense_slab_f32's.  One workspace serves one stream at a time.
 * ebos_iwe_dense_slab_multiref_f32: the accumulate pass over a grid of (work item, k) -- workgroup (tile, split, k) keeps ONE LDS
 *   window of tile + halo, fixed point with the exact f64 redo as in the single form, and writes its slab -- and the combine pass
 *   over (pixel block, k), which OVERWRITES iwes [K, H + 2 pad_h, W + 2 pad_w].  Two launches whatever K is.  Image k has the bits
 *   ebos_iwe_dense_slab_f32 gives on the same arrays with dts replaced by dt + shifts[k].  want_variance = 1: variances [K] (f32,
 *   nullable) and moments [K, 2] = (mean_k, M) (f64, nullable), omit_boundary as in the costs; 2: only the (sum, sum of squares)
 *   partials are left in each section (ebos_iwe_slab_partials gives their place inside a section); 0: neither.
 * ebos_iwe_dense_tiled_multiref_bwd_f32: d_flow[c][i] = sum over the events of source pixel i and the references k of
 *   -dt_k * dL/d(x'_k, y'_k) in ONE launch: one workgroup per tile keeps the two f64 planes of its tile's d_flow in LDS and sweeps
 *   the references -- stage G_k of tile + halo in LDS, walk the tile's events with dt_k, add -- then OVERWRITES d_flow [2, H, W]
 *   (+ addend [2, H, W], nullable) with plain stores: every cell, zeros where no event lies.  A source pixel's run is walked by
 *   one owner thread in plan order (runs of more than 64 events by its wavefront with a fixed reduction tree): no atomics, the
 *   same bits on every call.  Events whose taps leave the staged halo read G_k from global memory.  Upstream forms:
 *     g_images [K, h, w] with affine [K, 2] on the device (nullable: a = 1, c = 0):  G_k = a_k g_images[k] + c_k;
 *     var_moments [K, 2] (f64, the forward's moments) + upstream [1] (f32, device), both or neither, no affine: g_images are the
 *       IWEs themselves and G_k = scales[k] * upstream[0] * 2 (IWE_k - mean_k) / (M - 1); scales: HOST float [K], nullable (1);
 *     G_k = 0 outside [g_lo, h - g_lo) x [g_lo, w - g_lo).
 *   LDS: 2 tile_h tile_w 8 B + (tile_h + 2 halo)(tile_w + 2 halo) 4 B, the single backward's budget.
 * Both: the (x, y, dt) format of an emit = "full" binned plan (key_offsets of ebos_bin_events_f32, SoA arrays padded to 16-byte
 *   loads), unit weights, a dense flow [2, H, W], splits >= 1.  EBOS_ERR_UNSUPPORTED before any launch: splits = 0 (adaptive work
 *   items), halo < 0 (run-time windows), a triple that is not built.  The compact / fractional formats, per-event weights and the
 *   patch-grid-sampling route have no form here.
 * ---------------------------------------------------------------------------------------- */
int ebos_slab_multiref_config(int* out, int cap);
size_t ebos_iwe_slab_multiref_workspace_bytes(int K, int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w);
int ebos_iwe_dense_slab_multiref_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                     const float* flow, int H, int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w,
                                     const float* shifts, int K, void* workspace, size_t workspace_bytes, float* iwes, int want_variance,
                                     int omit_boundary, float* variances, double* moments, ebos_stream_t stream);
int ebos_iwe_dense_tiled_multiref_bwd_f32(const float* xs, const float* ys, const float* dts, const int32_t* key_offsets, int64_t n,
                                          const float* flow, int H, int W, int tile_h, int tile_w, int halo, int pad_h, int pad_w,
                                          const float* shifts, int K, const float* g_images, const float* affine, int g_lo,
                                          const double* var_moments, const float* upstream, const float* scales, const float* addend,
                                          float* d_flow, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The Adam loop of the MULTI-REFERENCE patch-flow contrast maximisation natively (the solver's `multi_reference` block with
 * `native: true`):
 *     loss(theta) = -(w_variance / (K norm)) sum_k var(IWE_k(dense(theta))) + w_flow_norm * flow_norm(dense)
 *                   + w_image_gradient * image_gradient(dense)
 * n_iter iterations enqueued back to back on `stream` by one C call: no host synchronisation, no allocation.  One iteration:
 *     ebos_upsample_patch_flow_f32 -> ebos_iwe_dense_slab_multiref_f32 (want_variance = 1) [-> ebos_flow_regularisers_f32]
 *     -> ebos_iwe_dense_tiled_multiref_bwd_f32 (var_moments, upstream, addend = regulariser gradient) -> a one-thread fold of the K
 *     variances into contrast[0] -> ebos_upsample_patch_flow_bwd_adam_f32 (contrast_scale = -w_variance / (K norm))
 * 7 launches per iteration, 8 with a regulariser weight, whatever K is.  All buffers are the caller's:
 *   plan:     xs / ys / dts in key order, key_offsets, n, H, W, tile, halo, splits (>= 1), pad, omit_boundary as
 *             ebos_iwe_dense_slab_multiref_f32; K and shifts[k] = f - r_k
 *   grid:     theta / d_theta / exp_avg / exp_avg_sq [2, gh, gw], step [1] int32, patch and sliding window, steps_done, theta_mask
 *             as in ebos_cmax_patch_problem
 *   images:   dense / d_dense [2, H, W], d_reg [2, H, W] (nullable iff both regulariser weights are 0), iwes [K, H + 2 pad_h,
 *             W + 2 pad_w], variances [K] f32, moments [K, 2] f64, contrast [1] f32, upstream [1] f32 = -w_variance / (K norm)
 *   norm:     N of the block's `normalize` (the contrast of the zero-flow IWE), 1 without it; finite and non-zero
 *   scratch:  workspace (ebos_iwe_slab_multiref_workspace_bytes, zero-filled once), reg_partials
 *             [ebos_flow_regularisers_partials()] f64, upsample_scratch (ebos_upsample_bwd_scratch_bytes)
 *   losses:   [losses_cap] f32, entry `step` written per iteration with the loss BEFORE the update (nullable)
 * Checked before any launch, reported through ebos_last_error: NULL pointers, K, sizes (EBOS_ERR_INVALID_ARG), an unbuilt
 * triple / splits = 0 / halo < 0 (EBOS_ERR_UNSUPPORTED), workspace_bytes and upsample_scratch_bytes (EBOS_ERR_SCRATCH).
 * ebos_cmax_multiref_gradient_f32: one forward and backward at theta without the Adam step -- d_theta, variances and reg_partials are
 *   left for the caller (loss = -(w_variance / (K norm)) sum(variances) + sum(reg_partials)); for optimisers that live on the host.
 * ---------------------------------------------------------------------------------------- */
typedef struct ebos_cmax_multiref_problem {
  const float *xs, *ys, *dts;
  const int32_t* key_offsets;
  int64_t n;
  int H, W, tile_h, tile_w, halo, pad_h, pad_w, omit_boundary, splits;
  int K;
  float shifts[EBOS_MULTIREF_MAX];
  int gh, gw, patch_h, patch_w, slide_h, slide_w;
  float w_variance, w_flow_norm, w_image_gradient;
  double norm;
  double lr, beta1, beta2, eps;
  float *theta, *d_theta, *exp_avg, *exp_avg_sq;
  int* step;
  int steps_done;
  float *dense, *d_dense, *d_reg, *iwes, *variances, *contrast;
  double* moments;
  const float* upstream;
  void* workspace;
  size_t workspace_bytes;
  double* reg_partials;
  float* upsample_scratch;
  size_t upsample_scratch_bytes;
  float* losses;
  int losses_cap;
  const float* theta_mask;
} ebos_cmax_multiref_problem;
int ebos_cmax_multiref_solve_f32(const ebos_cmax_multiref_problem* problem, int n_iter, ebos_stream_t stream);
int ebos_cmax_multiref_gradient_f32(const ebos_cmax_multiref_problem* problem, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The Adam loop of the TIME-AWARE patch-flow contrast maximisation natively (the solver's `time_aware` block):
 *     loss(theta) = -w_variance * var(IWE(events warped by voxel(dense(theta))))
 *                   + w_flow_norm * flow_norm(dense) + w_image_gradient * image_gradient(dense)
 * n_iter iterations enqueued back to back on `stream` by one C call: no host synchronisation, no allocation.  ONE window is a batch
 * of one: ebos_cmax_voxel_solve_f32 / _gradient_f32 copy the problem into an ebos_cmax_voxel_batch_problem (below) with B = 1,
 * n[0] = n and every other field under its own name, and run ebos_cmax_voxel_solve_batch_f32's code: its checks (a refusal names
 * ebos_cmax_voxel_solve / ebos_cmax_voxel_gradient), its sequence of stages, its results.  A NULL problem is refused first.
 * All buffers are the caller's:
 *   plan:     xs / ys / dts / bins in key order, key_offsets, n, H, W, tile, halo (a built halo; <= 0: the general forward kernel),
 *             pad, omit_boundary, splits (>= 1, as ebos_iwe_voxel_tiled_f32)
 *   voxel:    T in [1, 255], scheme EBOS_FLOW_UPWIND / _BURGERS, t0_index, wrap_last, route, has_clamp / clamp as
 *             ebos_flow_voxel_advect_f32; voxel [T, 2, H, W] receives the UNCLAMPED voxel, voxel_clamped (nullable unless
 *             has_clamp) the copy the events read; d_voxel [T, 2, H, W]; adjoint_workspace of
 *             ebos_flow_voxel_advect_adjoint_workspace(scheme, 1, T, H, W, t0_index, wrap_last, route) floats (nullable when 0)
 *   grid:     theta / d_theta / exp_avg / exp_avg_sq [2, gh, gw], step [1] int32, patch and sliding window, steps_done, theta_mask
 *             as in ebos_cmax_patch_problem
 *   images:   dense / d_dense [2, H, W], d_reg [2, H, W] (nullable iff both regulariser weights are 0), iwe [H + 2 pad_h,
 *             W + 2 pad_w], variance [1] f32, moments [2] f64, upstream [1] f32 = -w_variance, affine [2] f32
 *   scratch:  cost_scratch (ebos_cost_scratch_bytes(1)), reg_partials [ebos_flow_regularisers_partials()] f64,
 *             upsample_scratch (ebos_upsample_bwd_scratch_bytes)
 *   losses:   [losses_cap] f32, entry `step` written per iteration with the loss BEFORE the update (nullable)
 * ebos_cmax_voxel_gradient_f32: one forward and backward at theta without the Adam step -- d_theta, variance and reg_partials are
 *   left for the caller (loss = -w_variance * variance[0] + sum(reg_partials)); for optimisers that live on the host.
 * ---------------------------------------------------------------------------------------- */
typedef struct ebos_cmax_voxel_problem {
  const float *xs, *ys, *dts;
  const uint8_t* bins;
  const int32_t* key_offsets;
  int64_t n;
  int H, W, tile_h, tile_w, halo, pad_h, pad_w, omit_boundary, splits;
  int T, scheme, t0_index, wrap_last, route, has_clamp;
  double clamp;
  int owner_bwd;               /* 1: the pixel-owner backward; 0: memset + ebos_iwe_voxel_bwd_f32 (global float atomics) */
  int gh, gw, patch_h, patch_w, slide_h, slide_w;
  float w_variance, w_flow_norm, w_image_gradient;
  double lr, beta1, beta2, eps;
  float *theta, *d_theta, *exp_avg, *exp_avg_sq;
  int* step;
  int steps_done;
  float *dense, *d_dense, *d_reg, *voxel, *voxel_clamped, *d_voxel, *iwe, *variance;
  double* moments;
  const float* upstream;
  float* affine;
  void* cost_scratch;
  size_t cost_scratch_bytes;
  double* reg_partials;
  float* upsample_scratch;
  float* adjoint_workspace;
  int64_t adjoint_workspace_elems;
  float* losses;
  int losses_cap;
  const float* theta_mask;
} ebos_cmax_voxel_problem;
int ebos_cmax_voxel_solve_f32(const ebos_cmax_voxel_problem* problem, int n_iter, ebos_stream_t stream);
int ebos_cmax_voxel_gradient_f32(const ebos_cmax_voxel_problem* problem, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The time-aware loop for SEVERAL windows of one geometry per call: one Adam iteration of B windows runs in the launches of one
 * window, the window being an outer grid dimension of every stage.  Each window has its own events, patch grid and Adam state.
 *
 * The stacked plan: xs / ys / dts / bins are the windows' streams (key order) one after the other; key_offsets [B, n_keys + 1] int32
 * holds in row b window b's offsets shifted by the window's base, i.e. offsets INTO THE CONCATENATION, so the kernels need no pointer
 * table; ns [B] (HOST memory) the windows' event counts, whose sum is at most INT32_MAX.  A window with ns[b] = 0 is valid.
 *
 * The stages (each is the single entry point of the same name with the window dimension; per window the same arithmetic in the
 * same order, so on identical inputs the deterministic ones give the single call's bits):
 *   ebos_upsample_patch_flow_batch_f32       grid [B, 2, gh, gw] -> dense [B, 2, H, W]; grid.z = 2 B channels
 *   ebos_iwe_voxel_tiled_batch_f32           work item (tile, split, window): grid (tiles * splits, B); window b reads row b of
 *       the offsets and voxel[b] ([B, T, 2, H, W]) and ACCUMULATES into iwe[b] ([B, h, w]).  Every ebos_tiled_config is served;
 *       where (tile_h, tile_w, halo) is none, the general kernel ebos_iwe_voxel_f32 runs window by window.  No weights.
 *   ebos_iwe_voxel_owner_bwd_batch_f32       key (pixel key, window): grid (n_keys / 256, B); g_image [B, h, w], affine [B, 2]
 *       (nullable), d_voxel [B, T, 2, H, W] OVERWRITTEN.  A run is clamped to its own window's slice of the streams whatever the
 *       table holds.  Per window the properties of ebos_iwe_voxel_owner_bwd_f32: no atomics, every cell written, a fixed order of
 *       additions, hot pixels walked by the whole wave.
 *   ebos_flow_regularisers_batch_f32         flow / d_flow [B, 2, H, W], partials [B, ebos_flow_regularisers_partials()]
 *   ebos_upsample_patch_flow_bwd_batch_f32   d_dense [B, 2, H, W] -> d_grid [B, 2, gh, gw]; scratch of
 *       B * ebos_upsample_bwd_scratch_bytes(gh, W) bytes
 *   ebos_upsample_patch_flow_bwd_adam_batch_f32  ... + the Adam step of every window's grid (theta / exp_avg / exp_avg_sq
 *       [B, 2, gh, gw]) and the loss record: contrast [B], reg_partials [B, n_reg], grad_mask [B, gh, gw] (nullable),
 *       losses [B, losses_cap]; ONE step counter `step` [1] and one t for all windows.
 * ---------------------------------------------------------------------------------------- */
#define EBOS_CMAX_VOXEL_MAX_BATCH 64
int ebos_upsample_patch_flow_batch_f32(const float* grid, int B, int gh, int gw, int patch_h, int patch_w, int slide_h, int slide_w,
                                       int H, int W, float* dense, ebos_stream_t stream);
int ebos_iwe_voxel_tiled_batch_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                   const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H, int W,
                                   int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w, float* iwe,
                                   ebos_stream_t stream);
int ebos_iwe_voxel_owner_bwd_batch_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                       const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H, int W,
                                       int tile_h, int tile_w, int pad_h, int pad_w, const float* g_image, const float* affine,
                                       int g_lo, float* d_voxel, ebos_stream_t stream);
int ebos_flow_regularisers_batch_f32(const float* flow, int B, int H, int W, float w_flow_norm, float w_image_gradient, float* d_flow,
                                     double* partials, ebos_stream_t stream);
int ebos_upsample_patch_flow_bwd_batch_f32(const float* d_dense, int B, int gh, int gw, int patch_h, int patch_w, int slide_h,
                                           int slide_w, int H, int W, float* scratch, float* d_grid, ebos_stream_t stream);
int ebos_upsample_patch_flow_bwd_adam_batch_f32(const float* d_dense, int B, int gh, int gw, int patch_h, int patch_w, int slide_h,
                                                int slide_w, int H, int W, float* scratch, float* d_grid, float* theta, float* exp_avg,
                                                float* exp_avg_sq, double lr, double beta1, double beta2, double eps, int t, int* step,
                                                const float* contrast, float contrast_scale, const double* reg_partials, int n_reg,
                                                float* losses, int losses_cap, const float* grad_mask, ebos_stream_t stream);

/* ebos_cmax_voxel_solve_batch_f32: the loop's one implementation.  n_iter iterations, every stage called ONCE for all B windows
 * (one memset clears every IWE, one pass adds the regularisers' gradients); no host synchronisation, no allocation.  One iteration:
 *     ebos_upsample_patch_flow_batch_f32 -> ebos_flow_voxel_advect_f32 (unclamped; + ebos_flow_voxel_clamp_f32 with has_clamp)
 *     -> memset + ebos_iwe_voxel_tiled_batch_f32 (ebos_iwe_voxel_f32 window by window when (tile, halo) is no ebos_tiled_config)
 *     -> ebos_image_variance_f32 + ebos_image_variance_affine_f32 (upstream = -w_variance) [-> ebos_flow_regularisers_batch_f32]
 *     -> ebos_iwe_voxel_owner_bwd_batch_f32 (owner_bwd = 1) or one memset of d_voxel + ebos_iwe_voxel_bwd_f32 sorted, window by
 *        window (owner_bwd = 0)
 *     -> ebos_flow_voxel_advect_adjoint_f32 [-> d_dense += d_reg] -> ebos_upsample_patch_flow_bwd_adam_batch_f32
 * The fields are those of ebos_cmax_voxel_problem with the window dimension in front:
 *   plan:     B in [1, 64]; the stacked plan above, n[b] for b < B the windows' event counts
 *   grid:     theta / d_theta / exp_avg / exp_avg_sq [B, 2, gh, gw], theta_mask [B, gh, gw] (nullable), step [1], steps_done
 *   images:   dense / d_dense / d_reg [B, 2, H, W], voxel / voxel_clamped / d_voxel [B, T, 2, H, W], iwe [B, h, w],
 *             variance [B], moments [B, 2] f64, upstream [B] (each -w_variance), affine [B, 2]
 *   scratch:  cost_scratch of ebos_cost_scratch_bytes(B), reg_partials [B, ebos_flow_regularisers_partials()], upsample_scratch of
 *             B * ebos_upsample_bwd_scratch_bytes(gh, W), adjoint_workspace of
 *             ebos_flow_voxel_advect_adjoint_workspace(scheme, B, T, H, W, t0_index, wrap_last, route) floats
 *   losses:   [B, losses_cap]
 * Everything is validated before the first launch.  ebos_cmax_voxel_gradient_batch_f32: one forward and backward without the step. */
typedef struct ebos_cmax_voxel_batch_problem {
  int B;
  const float *xs, *ys, *dts;
  const uint8_t* bins;
  const int32_t* key_offsets;
  int64_t n[EBOS_CMAX_VOXEL_MAX_BATCH];
  int H, W, tile_h, tile_w, halo, pad_h, pad_w, omit_boundary, splits;
  int T, scheme, t0_index, wrap_last, route, has_clamp;
  double clamp;
  int owner_bwd;
  int gh, gw, patch_h, patch_w, slide_h, slide_w;
  float w_variance, w_flow_norm, w_image_gradient;
  double lr, beta1, beta2, eps;
  float *theta, *d_theta, *exp_avg, *exp_avg_sq;
  int* step;
  int steps_done;
  float *dense, *d_dense, *d_reg, *voxel, *voxel_clamped, *d_voxel, *iwe, *variance;
  double* moments;
  const float* upstream;
  float* affine;
  void* cost_scratch;
  size_t cost_scratch_bytes;
  double* reg_partials;
  float* upsample_scratch;
  float* adjoint_workspace;
  int64_t adjoint_workspace_elems;
  float* losses;
  int losses_cap;
  const float* theta_mask;
} ebos_cmax_voxel_batch_problem;
int ebos_cmax_voxel_solve_batch_f32(const ebos_cmax_voxel_batch_problem* problem, int n_iter, ebos_stream_t stream);
int ebos_cmax_voxel_gradient_batch_f32(const ebos_cmax_voxel_batch_problem* problem, ebos_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Time-aware warp at K <= EBOS_MULTIREF_MAX reference times (csrc/warp_voxel_multiref.hip): the flow voxel of the time-aware
 * entries above, scored at K reference times as the multi-reference entries score a dense flow.  The plan is binned, time-aware
 * and built with normalised time; reference k is the scalar shifts[k] = f - r_k (HOST memory, float [K], finite):
 *     dt_k = dt + shifts[k] (float32; shifts[k] == 0: dt as it is)
 *     x'_k = x - dt_k * voxel[bin][0][src],  y'_k = y - dt_k * voxel[bin][1][src];  the bin of an event does not depend on k.
 * The stacked plan, ns, B and the voxels [B, T, 2, H, W] are those of ebos_iwe_voxel_tiled_batch_f32.  No per-event weights.
 *   ebos_iwe_voxel_multiref_tiled_batch_f32      work item (tile, split, window, reference): grid (tiles * splits, B, K), ONE LDS
 *       window per workgroup, the body, accumulator rule and spill path (exact for any displacement) of ebos_iwe_voxel_tiled_f32.
 *       ACCUMULATES into iwes [B, K, h, w], which the caller zero-fills once.  Every ebos_tiled_config is served; where
 *       (tile_h, tile_w, halo) is none, the general global-atomic kernel runs window by window and reference by reference.
 *   ebos_iwe_voxel_multiref_owner_bwd_batch_f32  d_voxel[b][bin][c][i] = sum over the events e of window b with source pixel i and
 *       that bin, and over the references k, of -dt_k * dL/d(x', y')_{e,k}; the four taps are read from G_k = a_k * g_images[b][k] +
 *       c_k (g_images [B, K, h, w]; affine [B, K, 2] on the device, nullable: a = 1, c = 0), G_k = 0 outside
 *       [g_lo, h - g_lo) x [g_lo, w - g_lo).  The organisation of ebos_iwe_voxel_owner_bwd_batch_f32 -- one lane per source-pixel key,
 *       the three regimes of a run's length -- with the events loaded and their flow cells gathered ONCE and the references swept
 *       per chunk of events; an event's addend is summed over k = 0 .. K - 1 before the per-bin sums.  No atomics;
 *       d_voxel [B, T, 2, H, W] is OVERWRITTEN, every cell (zeros where nothing lands, empty windows included); the order of the
 *       additions is the plan's, so two calls give the same bits, and a window's bits do not depend on its place in the batch.
 *   ebos_iwe_voxel_multiref_tiled_f32 / ebos_iwe_voxel_multiref_owner_bwd_f32: one window -- the batch entries with B = 1
 *       (iwes [K, h, w], g_images [K, h, w], affine [K, 2], d_voxel [T, 2, H, W]).
 * Refused before any launch (EBOS_ERR_INVALID_ARG): K outside [1, EBOS_MULTIREF_MAX], NULL or non-finite shifts, and what the
 * single-reference entries refuse.
 * ---------------------------------------------------------------------------------------- */
int ebos_iwe_voxel_multiref_tiled_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                      const int32_t* key_offsets, int64_t n, const float* voxel, int T, int H, int W, int tile_h,
                                      int tile_w, int halo, int splits, int pad_h, int pad_w, const float* shifts, int K, float* iwes,
                                      ebos_stream_t stream);
int ebos_iwe_voxel_multiref_owner_bwd_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                          const int32_t* key_offsets, int64_t n, const float* voxel, int T, int H, int W, int tile_h,
                                          int tile_w, int pad_h, int pad_w, const float* shifts, int K, const float* g_images,
                                          const float* affine, int g_lo, float* d_voxel, ebos_stream_t stream);
int ebos_iwe_voxel_multiref_tiled_batch_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                            const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H,
                                            int W, int tile_h, int tile_w, int halo, int splits, int pad_h, int pad_w,
                                            const float* shifts, int K, float* iwes, ebos_stream_t stream);
int ebos_iwe_voxel_multiref_owner_bwd_batch_f32(const float* xs, const float* ys, const float* dts, const uint8_t* bins,
                                                const int32_t* key_offsets, const int64_t* ns, int B, const float* voxel, int T, int H,
                                                int W, int tile_h, int tile_w, int pad_h, int pad_w, const float* shifts, int K,
                                                const float* g_images, const float* affine, int g_lo, float* d_voxel,
                                                ebos_stream_t stream);

/* ebos_cmax_voxel_multiref_solve_batch_f32: the time-aware loop above scored at K reference times (the solver's `time_aware` block
 * with `directions` and `native: true`).  Per window
 *     loss(theta) = -(w_variance inv_norm / K) sum_k var(IWE_k(events warped by voxel(dense(theta)))) + the regularisers
 * through the stages of ebos_cmax_voxel_solve_batch_f32 -- its code -- on B K images:
 *     ebos_upsample_patch_flow_batch_f32 -> ebos_flow_voxel_advect_f32 [+ clamp] -> one memset of B K IWEs
 *     -> ebos_iwe_voxel_multiref_tiled_batch_f32 -> ebos_image_variance_f32 + ebos_image_variance_affine_f32 over B K images
 *     -> value[b] = inv_norm[b] * mean_k variance[b][k] (one small kernel) [-> ebos_flow_regularisers_batch_f32]
 *     -> ebos_iwe_voxel_multiref_owner_bwd_batch_f32 -> ebos_flow_voxel_advect_adjoint_f32 [-> d_dense += d_reg]
 *     -> ebos_upsample_patch_flow_bwd_adam_batch_f32 (contrast = value, contrast_scale = -w_variance)
 * The fields are ebos_cmax_voxel_batch_problem's, without owner_bwd (only the owner backward exists for K references), plus
 *   K, shifts:  1 <= K <= EBOS_MULTIREF_MAX reference times, shifts[k] = f - r_k (finite)
 *   inv_norm:   [B] f32 on the device, 1 / N of the block's `normalize` (N: the variance of the window's zero-flow IWE), 1 without it
 *   images:     iwe [B, K, h, w], variance [B, K] f32, moments [B, K, 2] f64, affine [B, K, 2] f32,
 *               upstream [B, K] f32 = -w_variance inv_norm[b] / K, value [B] f32
 *   scratch:    cost_scratch of ebos_cost_scratch_bytes(B K)
 * t0_index says where the base flow lives in the voxel and is independent of the reference times.  Refused before the first launch,
 * under the caller's entry-point name: a NULL problem, K outside [1, EBOS_MULTIREF_MAX], a non-finite shift, NULL inv_norm / value,
 * a cost_scratch too small for B K images (EBOS_ERR_SCRATCH), and everything ebos_cmax_voxel_solve_batch_f32 refuses.
 * ebos_cmax_voxel_multiref_gradient_batch_f32: one forward and backward at theta without the Adam step -- d_theta, value and
 *   reg_partials are left for the caller (loss[b] = -w_variance * value[b] + sum(reg_partials[b])). */
typedef struct ebos_cmax_voxel_multiref_batch_problem {
  int B;
  const float *xs, *ys, *dts;
  const uint8_t* bins;
  const int32_t* key_offsets;
  int64_t n[EBOS_CMAX_VOXEL_MAX_BATCH];
  int H, W, tile_h, tile_w, halo, pad_h, pad_w, omit_boundary, splits;
  int T, scheme, t0_index, wrap_last, route, has_clamp;
  double clamp;
  int K;
  float shifts[EBOS_MULTIREF_MAX];
  int gh, gw, patch_h, patch_w, slide_h, slide_w;
  float w_variance, w_flow_norm, w_image_gradient;
  double lr, beta1, beta2, eps;
  float *theta, *d_theta, *exp_avg, *exp_avg_sq;
  int* step;
  int steps_done;
  float *dense, *d_dense, *d_reg, *voxel, *voxel_clamped, *d_voxel, *iwe, *variance;
  double* moments;
  const float* upstream;
  float* affine;
  const float* inv_norm;
  float* value;
  void* cost_scratch;
  size_t cost_scratch_bytes;
  double* reg_partials;
  float* upsample_scratch;
  float* adjoint_workspace;
  int64_t adjoint_workspace_elems;
  float* losses;
  int losses_cap;
  const float* theta_mask;
} ebos_cmax_voxel_multiref_batch_problem;
int ebos_cmax_voxel_multiref_solve_batch_f32(const ebos_cmax_voxel_multiref_batch_problem* problem, int n_iter, ebos_stream_t stream);
int ebos_cmax_voxel_multiref_gradient_batch_f32(const ebos_cmax_voxel_multiref_batch_problem* problem, ebos_stream_t stream);

/* ---- the stacked plan above for B windows, built from the raw sensor columns in one set of launches (csrc/plan_time_aware.hip) ----
 * col / row int16, t int32 (t_is_64 = 0) or int64 ticks: device columns of n_total events.  ranges: HOST int64 [B, 2], window b =
 * events [begin, end) of the columns; the ranges may overlap, come in any order and be empty.  An event is kept when it lies inside
 * the CROP rectangle (has_roi: rows [xmin, xmax), columns [ymin, ymax)), outside the removal rectangle (has_remove: rows
 * [rm_x0, rm_x1), columns [rm_y0, rm_y1)) -- the rectangles of ebos_window_ingest_raw_batch -- and its pixel lies inside the image.
 * Per window, what ebos_raw_time_range + ebos_raw_events_to_soa + ebos_event_time_bins_f64 + ebos_bin_events_f32 leave for the
 * events that pass the rectangles: tminmax[b] = the tick range of those events / ticks_per_second (float64; 0, 0 for none), dt by
 * the expression of ebos_raw_events_to_soa (float64, one rounding), bin by the rule of ebos_event_time_bins on
 * (double)ticks / ticks_per_second, x = (float)row, y = (float)col, sorted by the tile-major source key.  Outputs:
 *   xs, ys, dts float, bins uint8, perm int32 [capacity]  window b's kept events are the slice [base_b, base_b + n_b), base_b = the
 *       kept events of the earlier windows; perm = the event's index inside its range (col[begin + perm[i]] is its source).
 *       Only [0, sum n_b) is written.  capacity >= the sum of the range lengths.
 *   key_offsets_local, key_offsets_stacked int32 [B, key_stride], key_stride >= n_keys + 1: the window's own offsets, and
 *       local + base_b (the table of the batched kernels above when key_stride = n_keys + 1); an empty window's rows are constant.
 *   counts int32 [B, 2]: kept events, events that pass the rectangles but lie outside the image.
 * The order of the events of one source pixel is unspecified (as ebos_bin_events_f32).  Nine launches whatever B is, no host
 * synchronisation.  Validated before the first launch: 1 <= B <= EBOS_CMAX_VOXEL_MAX_BATCH, 1 <= T <= 255, H, W <= 32767, the
 * pointers, ranges inside n_total, at most INT32_MAX events in total, rectangle order (EBOS_ERR_INVALID_ARG), the scratch size
 * (EBOS_ERR_SCRATCH).  scratch: ebos_plan_time_aware_batch_scratch_bytes(ranges, B, H, W, tile_h, tile_w) bytes (0: bad arguments).
 * ---------------------------------------------------------------------------------------- */
size_t ebos_plan_time_aware_batch_scratch_bytes(const int64_t* ranges, int B, int H, int W, int tile_h, int tile_w);
int ebos_plan_time_aware_raw_batch(const int16_t* col, const int16_t* row, const void* t, int t_is_64, double ticks_per_second,
                                   int64_t n_total, const int64_t* ranges, int B, int has_roi, int xmin, int xmax, int ymin, int ymax,
                                   int has_remove, int rm_x0, int rm_x1, int rm_y0, int rm_y1, int ref_mode, double ref_fraction,
                                   int normalize_t, int T, int H, int W, int tile_h, int tile_w, float* xs, float* ys, float* dts,
                                   uint8_t* bins, int32_t* perm, int64_t capacity, int32_t* key_offsets_local,
                                   int32_t* key_offsets_stacked, int64_t key_stride, int32_t* counts, double* tminmax, void* scratch,
                                   size_t scratch_bytes, ebos_stream_t stream);

/* ---- Prophesee EVT 3.0 recordings: the 16-bit word stream of a .raw file decoded on the device (csrc/evt3.hip) ----
 * The reference's recordings are prophesee_0/cd_events.raw (src/data_loader/ccs.py:171); its own .raw path (:103-108, :299-317) is
 * switched off in favour of a conversion to HDF5 (:19-20).  A word's type is its bits 15..12, v its bits 11..0:
 *   0x8 TIME_HIGH    if the previous TIME_HIGH's value prev > v and prev - v >= 4085: loops += 1; then th = v, tl = 0
 *   0x6 TIME_LOW     tl = v
 *   0x0 ADDR_Y       y = v & 0x7FF
 *   0x2 ADDR_X       one event: x = v & 0x7FF, p = v >> 11
 *   0x3 VECT_BASE_X  bx = v & 0x7FF, pol = v >> 11
 *   0x4 VECT_12      an event at x = bx + b, polarity pol, for every set bit b of v, ascending; then bx += 12
 *   0x5 VECT_8       the same for bits 0..7; then bx += 8
 *   0xA EXT_TRIGGER  one trigger record: value = v & 1, id = v >> 8
 *   every other type is ignored
 * An event or trigger carries the row y and the time t = (loops << 24) | (th << 12) | tl microseconds.  The state starts all zero,
 * and every word before the first TIME_HIGH is ignored altogether: it emits nothing and sets nothing.  bx is kept modulo 2^16 (x is
 * an int16 column, the bit pattern of bx + b).  All arithmetic is integer and there is no atomic in the data path: the output is in
 * stream order and identical from run to run.
 *
 * A slab of n_words words is cut into chunks of ebos_evt3_chunk_words() words.  ebos_evt3_scan reduces every chunk to its state
 * transformer (one workgroup per chunk) and combines them in order from *carry_in (one small launch): every chunk's incoming state
 * and exclusive event / trigger offsets stay in `scratch`, totals[0 .. 1] = the slab's events and triggers, *carry_out = the state
 * after the slab's last word -- all on the device; carry_in NULL = the start state, carry_out may be carry_in.  The caller reads
 * `totals` back, allocates, and ebos_evt3_emit (one workgroup per chunk) decodes the SAME words again from that scratch into
 *   x, y int16, t int64, p uint8 [event_capacity];  trig_t int64, trig_value, trig_id uint8 [trigger_capacity]
 * and writes elements [0, n_events) and [0, n_triggers) only.  n_events / n_triggers are the totals as the caller read them; a
 * capacity below them is refused (EBOS_ERR_INVALID_ARG) before anything is written, and no store ever lands at or beyond a capacity.
 * NULL pointers (words may be NULL when n_words is 0; an output may be NULL when its capacity is 0), negative sizes, n_words beyond
 * 2^30 and a short scratch (EBOS_ERR_SCRATCH) are refused before any HIP call.  ebos_evt3_scratch_bytes: 0 for a bad n_words. */
typedef struct ebos_evt3_state {
  int32_t has_th; /* a TIME_HIGH has been seen */
  int32_t th, tl, y, bx, pol;
  int64_t loops;
} ebos_evt3_state;
int ebos_evt3_chunk_words(void);
size_t ebos_evt3_scratch_bytes(int64_t n_words);
int ebos_evt3_scan(const uint16_t* words, int64_t n_words, const ebos_evt3_state* carry_in, ebos_evt3_state* carry_out,
                   int64_t* totals, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_evt3_emit(const uint16_t* words, int64_t n_words, const void* scratch, size_t scratch_bytes, int64_t n_events,
                   int64_t n_triggers, int64_t event_capacity, int64_t trigger_capacity, int16_t* x, int16_t* y, int64_t* t,
                   uint8_t* p, int64_t* trig_t, uint8_t* trig_value, uint8_t* trig_id, ebos_stream_t stream);

/* ---- Prophesee EVT 2.0, EVT 2.1 and DAT recordings decoded on the device (csrc/evt2.hip; the state algebra: csrc/evt2_core.h) ----
 * The other formats Prophesee cameras and tools write.  The rules are written from the format documentation, not checked against
 * OpenEB.
 * EVT 2.0: little-endian uint32 words, type = w >> 28:
 *   0x8 EVT_TIME_HIGH  v = w & 0x0FFFFFFF; if the previous TIME_HIGH's value prev > v and prev - v >= 2^28 - 11: loops += 1; then th = v
 *   0x0 CD_OFF, 0x1 CD_ON  one event: p = type, ts = (w >> 22) & 0x3F, x = (w >> 11) & 0x7FF, y = w & 0x7FF
 *   0xA EXT_TRIGGER    one trigger record: ts = (w >> 22) & 0x3F, id = (w >> 8) & 0x1F, value = w & 1
 *   every other type is ignored (0xE OTHERS and 0xF CONTINUED included)
 * EVT 2.1: little-endian uint64 words, type = w >> 60:
 *   0x8 EVT_TIME_HIGH  v = (w >> 32) & 0x0FFFFFFF, the same loop rule
 *   0x0 EVT_NEG, 0x1 EVT_POS  p = type, ts = (w >> 54) & 0x3F, bx = (w >> 43) & 0x7FF, y = (w >> 32) & 0x7FF, valid = w & 0xFFFFFFFF:
 *                      an event at x = bx + b for every set bit b of valid, ascending (x is the int16 bit pattern: bx + 31 reaches 2078)
 *   0xA EXT_TRIGGER    ts = (w >> 54) & 0x3F, id = (w >> 40) & 0x1F, value = (w >> 32) & 1
 *   every other type is ignored
 *   half_swapped != 0: the legacy order, the two 32-bit halves of every word exchanged in the file; undone as the words are loaded.
 * In both, an event or trigger carries t = (loops << 34) | (th << 6) | ts microseconds; the state starts all zero and every word
 * before the first TIME_HIGH is ignored altogether.  Integer arithmetic only, no atomic in the data path: stream order, the same
 * bytes every run.
 *
 * The protocol is that of ebos_evt3_scan / ebos_evt3_emit above, with word_bytes = 4 (EVT 2.0) or 8 (EVT 2.1): n_words counts
 * words of that size (at most 2^30), a slab is cut into chunks of ebos_evt2_chunk_words(word_bytes) words (0: bad word_bytes),
 * ebos_evt2_scan leaves every chunk's record, incoming state and exclusive offsets in `scratch`
 * (ebos_evt2_scratch_bytes(n_words, word_bytes) bytes; 0: bad arguments), totals[0 .. 1] = the slab's events and triggers (64-bit)
 * and *carry_out (carry_in NULL = the start state; carry_out may be carry_in), and ebos_evt2_emit decodes the SAME words again into
 * elements [0, n_events) and [0, n_triggers) of the seven columns of ebos_evt3_emit.  Refused before any HIP call
 * (EBOS_ERR_INVALID_ARG): a word_bytes other than 4 or 8, NULL pointers (words may be NULL when n_words is 0; an output when its
 * capacity is 0), words not aligned to word_bytes, negative sizes, n_words beyond 2^30, a capacity below the totals; a short
 * scratch: EBOS_ERR_SCRATCH.  No store lands at or beyond a capacity. */
typedef struct ebos_evt2_state {
  int32_t has_th; /* a TIME_HIGH has been seen */
  int32_t th;
  int64_t loops;
} ebos_evt2_state;
int ebos_evt2_chunk_words(int word_bytes);
size_t ebos_evt2_scratch_bytes(int64_t n_words, int word_bytes);
int ebos_evt2_scan(const void* words, int64_t n_words, int word_bytes /* 4 | 8 */, int half_swapped, const ebos_evt2_state* carry_in,
                   ebos_evt2_state* carry_out, int64_t* totals, void* scratch, size_t scratch_bytes, ebos_stream_t stream);
int ebos_evt2_emit(const void* words, int64_t n_words, int word_bytes, int half_swapped, const void* scratch, size_t scratch_bytes,
                   int64_t n_events, int64_t n_triggers, int64_t event_capacity, int64_t trigger_capacity, int16_t* x, int16_t* y,
                   int64_t* t, uint8_t* p, int64_t* trig_t, uint8_t* trig_value, uint8_t* trig_id, ebos_stream_t stream);
/* DAT: n_records records of two little-endian uint32 (ts, data), 8-byte aligned.  version 2: x = data & 0x3FFF, y = (data >> 14) &
 * 0x3FFF, p = (data >> 28) & 1; version 1: x = data & 0x1FF, y = (data >> 9) & 0xFF, p = (data >> 17) & 1; t = ts as it stands (no
 * wrap is counted).  Writes elements [0, n_records) of x, y int16, t int64, p uint8 [capacity]; one launch.  Refused before any HIP
 * call: n_records outside [0, 2^30], a version other than 1 or 2, capacity below n_records, NULL or misaligned pointers. */
int ebos_dat_decode(const void* records, int64_t n_records, int version, int16_t* x, int16_t* y, int64_t* t, uint8_t* p, int64_t capacity,
                    ebos_stream_t stream);

/* ---- photometric check of a flow: frame warp, SSIM and the fused per-item score (csrc/photometric.hip) ----
 * Element type codes of images, shifts and flows. */
#define EBOS_IMAGE_U8 0
#define EBOS_IMAGE_F32 1
#define EBOS_IMAGE_F64 2
/* The reference's warp_image_forward / warp_image_torch (src/utils/frame_utils.py:56-115) for B items: out[b] (H x W, the compute
 * type) = images[b] sampled at x - flow, bilinear, zeros outside, through the reference's chain -- the float32 base grid
 * i / ((size - 1) / 2) - 1, the displacement subtracted in its own type, grid_sample's align_corners=True un-normalisation, four
 * taps.  images: contiguous H x W planes of image_dtype (EBOS_IMAGE_U8 or the compute type), item b at element offset
 * b * image_sb (0: one image for all items).  Exactly one of flows ([B, 2, H, W], rows first, contiguous, the compute type) and
 * shifts ([B, 2] of shift_dtype: EBOS_IMAGE_F32 or the compute type; shift / ((size - 1) / 2) is formed in the shift's type and
 * subtracted from the grid in float32, as warp_image_torch's 0-dim shift is)
 * is given.  Refused before any launch (EBOS_ERR_INVALID_ARG): B outside 1 .. 65535, H or W below 2, H W >= 2^31, a NULL buffer,
 * a dtype code that is not built.  One launch. */
int ebos_warp_image_forward_f32(const void* images, int image_dtype, int64_t image_sb, const float* flows, const void* shifts,
                                int shift_dtype, int B, int H, int W, float* out, ebos_stream_t stream);
int ebos_warp_image_forward_f64(const void* images, int image_dtype, int64_t image_sb, const double* flows, const void* shifts,
                                int shift_dtype, int B, int H, int W, double* out, ebos_stream_t stream);
/* The reference's SSIM map (src/utils/stat_utils.py:228-243) of the B C image pairs img1[n], img2[n] (contiguous [B, C, H, W]):
 * the five moments E[x], E[y], E[x x], E[y y], E[x y] under taps (window_size x window_size of the compute type, made by the host
 * as create_window makes them), zero padding of window_size / 2, C1 = 0.01^2, C2 = 0.03^2.  out: [B, C, H, W].  means: NULL, or
 * ebos_ssim_means_elems(dtype, B, C, H, W) float64 (0: bad arguments): the mean of every map, of every item's C maps and of all maps --
 * the first B C + B + 1 values; the rest is scratch -- each the exact float64 sum rounded once, then divided (the map kernel leaves a
 * sum per tile; two more small launches).
 * Refused before any launch: B C outside 1 .. 65535, H or W below 2, H W >= 2^31, an even or non-positive window_size, a NULL
 * buffer (EBOS_ERR_INVALID_ARG); a window_size above ebos_photometric_max_window() (EBOS_ERR_UNSUPPORTED). */
int ebos_ssim_map_f32(const float* img1, const float* img2, const float* taps, int window_size, int B, int C, int H, int W, float* out,
                      double* means, ebos_stream_t stream);
int ebos_ssim_map_f64(const double* img1, const double* img2, const double* taps, int window_size, int B, int C, int H, int W, double* out,
                      double* means, ebos_stream_t stream);
int ebos_photometric_max_window(void);
size_t ebos_ssim_means_elems(int dtype, int B, int C, int H, int W);
/* The fused score of B items.  w = warp_image_forward(frame1[b], flow[b]) over the whole image.  A pixel is COUNTED when it lies in
 * rows [xmin, xmax) x columns [ymin, ymax) (has_roi), mask[b] is non-zero there (mask not NULL), both flow components are finite
 * and all four bilinear taps lie inside the image.  out [B, 7] float64:
 *   L1 = mean |w - frame2|, RMSE = sqrt(mean (w - frame2)^2), SSIM = mean of the SSIM map of (w, frame2)   over the counted pixels,
 *   L1_0, RMSE_0, SSIM_0 = the same with w = frame1,  n_points = the count (0: the other six are NaN).
 * dtype: the type of flow [B, 2, H, W] and taps, and the compute type (EBOS_IMAGE_F32 / _F64); frame_dtype: EBOS_IMAGE_U8 or dtype.
 * frame1: item b at element offset b * frame1_sb (0: shared); frame2 [B, H, W]; mask uint8, item b at b * mask_sb.  Two launches,
 * no atomics, no host synchronisation; the same bits on every run and wherever an item stands in the batch.  scratch:
 * ebos_photometric_scratch_bytes(dtype, B, H, W) bytes (0: bad arguments; EBOS_ERR_SCRATCH when short).  Refusals as above. */
size_t ebos_photometric_scratch_bytes(int dtype, int B, int H, int W);
int ebos_photometric_batch(int dtype, int frame_dtype, int B, int H, int W, const void* frame1, int64_t frame1_sb, const void* frame2,
                           const void* flow, const void* taps, int window_size, int has_roi, int xmin, int xmax, int ymin, int ymax,
                           const uint8_t* mask, int64_t mask_sb, double* out, void* scratch, size_t scratch_bytes, ebos_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EBOS_HIP_H */
