/*
 * sgn_rast.h — C ABI of libsgnrast.so, the MI355X (gfx950) differentiable
 * 3D-Gaussian rasterizer behind the gsplat `project_gaussians` /
 * `rasterize_gaussians` / `spherical_harmonics` surface that
 * street-gaussians-ns calls (sgn_splatfacto.py:860,939,954,982;
 * sgn_splatfacto_scene_graph.py:285).
 *
 * Every entry point replaces one function of the reference's FFI for this path,
 * i.e. of gsplat 0.1.x's `gsplat.cuda._C` pybind module (`gsplat/cuda/csrc/
 * bindings.cu`; third-party, not vendored in /root/reference — names below are
 * the upstream binding names).  Plain pointers + sizes, no torch types, no
 * exceptions, no mutable global state besides a thread-local error string and the opt-in profiling spans
 * (sgn_timing_*, off by default).
 *
 * Conventions
 *   - all pointers are DEVICE pointers to contiguous arrays unless marked host;
 *     fp32 unless noted; quats are (w,x,y,z); viewmat is the 3x4 row-major
 *     world->camera matrix (12 floats); images are [H,W,C] row-major.
 *   - `stream` is a hipStream_t (0 = default stream).  Calls only enqueue work.
 *   - workspaces are caller-allocated (torch caching allocator on the Python
 *     side) and sized by the matching *_workspace_bytes() query.
 *   - return 0 on success, <0 for an argument error, >0 = hipError_t;
 *     sgn_last_error() gives the message for the calling thread.
 */
#ifndef SGN_RAST_H
#define SGN_RAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *sgn_stream_t; /* hipStream_t */

#define SGN_RECORD_FLOATS 12 /* one packed intersection record = 48 bytes */

int sgn_version(void);
const char *sgn_last_error(void);

/* UPSTREAM-VARIANT SEMANTICS (round 6).  gsplat is not vendored by the reference and not installable where this library
 * is built: three behaviours of gsplat 0.1.x are DECIDED here from recollection of upstream, not read
 * from its source (SURVEY.md Appendix A marks them [verify] / [decide]).  Each is an ARGUMENT of the calls it touches,
 * with the decided behaviour as the default (0), so that a mismatch found by running tests/golden/make_upstream_golden.py
 * against the real gsplat is a flag flip in the caller, not a rewrite:
 *   `semantics` bit SGN_SEM_BBOX_ADD_AFTER_CAST   tile bbox max side = (int)(c + r) + 1 (gsplat/_torch_impl.py
 *        get_tile_bbox) instead of the default (int)(c + r + 1) (gsplat helpers.cuh get_bbox).  Differs only for
 *        -1 < c + r < 0: a splat whose 3-sigma box ends within one tile LEFT of / ABOVE the image is culled by the
 *        default and listed in tile column / row 0 by the variant.  Carried by every call that computes tile boxes:
 *        sgn_project_fwd*, sgn_map_isect, sgn_bin_prepare, sgn_rasterize_fwd_all, sgn_rasterize_window_all.
 *   `semantics` bit SGN_SEM_EWA_VJP_CLAMPED       the projection backward differentiates THROUGH the forward's
 *        +-1.3 tan(fov/2) clamp of (x/z, y/z) (what autograd through gsplat/_torch_impl.py gives) instead of the
 *        default, upstream CUDA's project_cov3d_ewa_vjp, which recomputes the Jacobian from the UN-clamped point.
 *        Carried by sgn_project_bwd* (which then need the image size: img_h, img_w).
 *   alpha_clamp_bwd (a float argument of sgn_raster_bwd*)   0.99f = upstream's backward clamp (default of the host
 *        side); 0.999f = the forward's.
 */
#define SGN_SEM_DEFAULT 0
#define SGN_SEM_BBOX_ADD_AFTER_CAST 1
#define SGN_SEM_EWA_VJP_CLAMPED 2

/* Kernel-selection options of the raster entry points, passed WITH EVERY CALL (NULL = the defaults): the library keeps
 * no mutable configuration of its own, so two threads / streams may rasterize with different settings.  (Round 1 had
 * process-global sgn_set_* switches here; they are gone.) */
typedef struct sgn_raster_opts {
    int exact_exp;      /* parity tests: 1 = portable polynomial exp (bit-identical to oracle/c/sgn_oracle.c
                           exp_portable), 0 (default) = hardware v_exp_f32 */
    int reduce_mode;    /* backward wave reduction: 1 (default) = transposed reduction on v_permlane32_swap /
                           v_permlane16_swap + DPP row adds (8 swaps + 12 DPP adds for the nine per-Gaussian sums);
                           0 = nine butterfly reductions (54 shuffles): an independent second form, run by the tests */
    int adapt_fwd, adapt_bwd; /* forward: lists of at least adapt_fwd entries (the head of the launch order) get four waves
                                 per tile instead of two; backward: reverse walks of at least adapt_bwd entries go to the
                                 four-waves-per-tile kernel (one wave per tile means ONE gradient reduction per (tile,
                                 Gaussian), four waves mean four).  Defaults 1024 / 256; <= 0 = default */
    int batch_fwd, batch_bwd; /* lists / reverse walks with at least this many entries are read through 64-entry
                                 batches staged in wave-private LDS instead of the one-entry scalar look-ahead
                                 (defaults 256 / 128; <= 0 = default; a huge value disables) */
    int debug_flags;    /* timing ablations for profiles/ ONLY (results become wrong): bit0 = no gradient atomics,
                           bit1 = no wave reduction; 0 = normal operation */
    int ids_qmask;      /* 1: gaussian_ids_sorted carries quadrant masks in bits 28-31 (sgn_bin_intersect with
                           quadrant_masks) — a property of the list handed in, not a tuning knob; default 0 */
} sgn_raster_opts;
/* (Round 6 removed what rounds 2-5 measured and lost: the "stream" mode `gather = 0`, the forced one- / four-wave shapes
 * `waves_fwd` / `waves_bwd`, `xcd_swizzle`, and `reduce_mode = 2`, the reduction's first stages on the matrix pipe —
 * profiles/experiments/ keeps their notes and numbers.) */
void sgn_raster_default_opts(sgn_raster_opts *out);

/* Opt-in per-kernel timing for bench.py / profiles: when enabled, each timed launch is bracketed by
 * hipEventRecord on the stream it is launched on; sgn_timing_get sums the finished spans of a slot. */
#define SGN_T_PROJECT_FWD 0
#define SGN_T_PROJECT_BWD 1
#define SGN_T_SH_FWD 2
#define SGN_T_SH_BWD 3
#define SGN_T_SCAN 4
#define SGN_T_MAP 5
#define SGN_T_SORT 6
#define SGN_T_BINS 7
#define SGN_T_PACK 8
#define SGN_T_RASTER_FWD 9
#define SGN_T_RASTER_BWD 10
#define SGN_T_UNPACK 11
#define SGN_T_SKY_FWD 12
#define SGN_T_SKY_BWD 13
#define SGN_T_LOSS_FWD 14
#define SGN_T_LOSS_BWD 15
#define SGN_T_ADAM 16
#define SGN_T_SLOTS 17
void sgn_timing_enable(int on); /* also clears recorded spans */
int sgn_timing_get(int slot, int *count /*host*/, float *total_ms /*host*/);
/* Host microseconds the CALLING THREAD has spent blocked in the waits (polled words, events) of the one-call entries (the quats check of
 * sgn_project_fwd_all / sgn_project_check_wait, the count of sgn_rasterize_fwd_all, the verdict of
 * sgn_rasterize_window_all) since the last reset; *n_waits (may be NULL) = how many waits.  Always on (two clock reads
 * per wait, thread-local): tells a profile whether a composite call's host time is its launches or its wait. */
double sgn_timing_host_wait_us(int reset, int64_t *n_waits /*host*/);

/* _C.project_gaussians_forward (gsplat/project_gaussians.py:_ProjectGaussians.forward;
 * reference call site sgn_splatfacto.py:860-873).  Every output row is written
 * (zeros for culled Gaussians), so the caller need not pre-zero. */
int sgn_project_fwd(int n, const float *means3d, const float *scales, float glob_scale,
                    const float *quats, const float *viewmat12, float fx, float fy, float cx,
                    float cy, int img_h, int img_w, int block_width, float clip_thresh,
                    float *cov3d /*[n,6]*/, float *xys /*[n,2]*/, float *depths /*[n]*/,
                    int32_t *radii /*[n]*/, float *conics /*[n,3]*/, float *compensation /*[n]*/,
                    int32_t *num_tiles_hit /*[n]*/, int semantics /*SGN_SEM_* bits; 0 = default*/, sgn_stream_t stream);

/* gsplat's `assert (quats.norm(dim=-1) - 1 < 1e-6).all()` (project_gaussians.py) as a device-side check: *flag (device
 * int32) becomes 1 if any row of quats [n,4] (16-byte aligned) fails `norm - 1 < tol`.  The host reads the flag at its
 * next sync point (see sgn_rast/ops.py: deferred assertion). */
int sgn_check_unit_quats(int n, const float *quats, float tol, int32_t *flag, sgn_stream_t stream);

/* `project_gaussians` as ONE call (round 5; no upstream counterpart): sgn_project_fwd with upstream's quats assertion
 * riding the projection kernel (check_quats != 0: a row of quats [n,4] that fails `norm - 1 < quat_tol`
 * STAMPS *flag_dev; the flag is copied to flag_pinned[0] behind the kernel), and — gid_by_rank != NULL — sgn_depth_rank
 * of the coming binning, all queued on `stream`; only then does the call wait for the flag and report *quats_bad_host
 * (1: some row failed; the host raises upstream's assertion).
 * flag_pinned: pinned host int32[3], or NULL (a pageable copy; check_quats = 1 only).  [0] = the stamp if a row failed,
 * [1] = the stamp once the launch's stores have landed (round 6): the wait refuses to report "normalized" — error -8 —
 * if [1] never shows the stamp; [2] = the stamp once the projection kernel is COMPLETE, stored by a one-wave kernel
 * queued behind it — the word the host POLLS instead of waiting for an event (no barrier packet on the stream) — or
 * -stamp where the slot is not mapped and a copy command + event are the transport.
 * flag_stamp > 0: the value a failing row stores; the caller guarantees *flag_dev / the slot holds no value >= flag_stamp
 * when the kernel runs (a word zeroed once, a counter per call on it), and nothing is cleared per call.  flag_stamp <= 0:
 * the call clears the flag itself (one more launch) and stamps 1.  rank_ws: sgn_depth_rank_workspace_bytes(n).
 * Where flag_pinned is mapped into the device's address space (hipHostMalloc'd memory is) and flag_stamp > 0, the kernel
 * stores both words straight into it (system-scope atomic stores) and no copy command is queued (flag_dev may then be
 * NULL).
 * check_quats = 2: everything is queued as above but the call does NOT wait (flag_pinned required, quats_bad_host unused):
 * the caller finishes its own host-side bookkeeping and then calls sgn_project_check_wait — same thread, same device —
 * which polls flag_pinned[2] (or waits for the check's own event) and reports the flag; `stream`: the stream of the
 * sgn_project_fwd_all call (drained once if the word has not arrived after 0.2 s: the cold path). */
int sgn_project_fwd_all(int n, const float *means3d, const float *scales, float glob_scale, const float *quats,
                        const float *viewmat12, float fx, float fy, float cx, float cy, int img_h, int img_w,
                        int block_width, float clip_thresh, float *cov3d, float *xys, float *depths, int32_t *radii,
                        float *conics, float *compensation, int32_t *num_tiles_hit, int check_quats, float quat_tol,
                        int32_t *flag_dev, int32_t flag_stamp, int32_t *flag_pinned, int32_t *gid_by_rank,
                        void *rank_ws, size_t rank_ws_bytes, int sort_rank_mode, int32_t *quats_bad_host,
                        int semantics, sgn_stream_t stream);

int sgn_project_check_wait(const int32_t *flag_pinned, int32_t flag_stamp, int32_t *quats_bad_host /*host*/,
                           sgn_stream_t stream);

/* _C.project_gaussians_backward (_ProjectGaussians.backward).  v_compensation may be NULL
 * (treated as zeros: the reference discards compensation, sgn_splatfacto.py:860,947); v_depth may be NULL too
 * (zeros: depths took no part in the loss).
 * v_cov2d / v_cov3d are optional scratch outputs (may be NULL).  All rows written. */
int sgn_project_bwd(int n, const float *means3d, const float *scales, float glob_scale,
                    const float *quats, const float *viewmat12, float fx, float fy,
                    const float *cov3d, const int32_t *radii, const float *conics,
                    const float *compensation, const float *v_xy, const float *v_depth,
                    const float *v_conic, const float *v_compensation, float *v_cov2d,
                    float *v_cov3d, float *v_mean3d, float *v_scale, float *v_quat,
                    int semantics /*SGN_SEM_EWA_VJP_CLAMPED: needs img_h, img_w*/, int img_h, int img_w,
                    sgn_stream_t stream);

/* Fused front ends (extensions beyond gsplat's surface; SURVEY.md §8 a8, BASELINE.json north_star:
 * "projection with the scene-graph's per-object rigid transform fused in").  Same outputs as
 * sgn_project_fwd/bwd applied to  means_w = R_o m + t_o,  quats = normalize(q_o2w (x) q_raw),
 * scales = exp(log_scales)  (sgn_splatfacto_scene_graph.py:404-417, sgn_splatfacto.py:857,864), and the
 * gradients are returned w.r.t. the LOCAL means, the LOG scales and the RAW quaternions.
 * poses: [n_objects,16] floats per row = R row-major (9), t (3), q_o2w wxyz (4); object_ids/poses may
 * both be NULL (no rigid transform, activations only). */
int sgn_project_fwd_fused(int n, const float *means_local, const float *log_scales, float glob_scale,
                          const float *quats_raw, const int32_t *object_ids, const float *poses,
                          const float *viewmat12, float fx, float fy, float cx, float cy, int img_h,
                          int img_w, int block_width, float clip_thresh, float *cov3d, float *xys,
                          float *depths, int32_t *radii, float *conics, float *compensation,
                          int32_t *num_tiles_hit, int semantics, sgn_stream_t stream);
int sgn_project_bwd_fused(int n, const float *means_local, const float *log_scales, float glob_scale,
                          const float *quats_raw, const int32_t *object_ids, const float *poses,
                          const float *viewmat12, float fx, float fy, const float *cov3d,
                          const int32_t *radii, const float *conics, const float *compensation,
                          const float *v_xy, const float *v_depth, const float *v_conic,
                          const float *v_compensation, float *v_means_local, float *v_log_scales,
                          float *v_quats_raw, int semantics, int img_h, int img_w, sgn_stream_t stream);

/* sgn_project_bwd_fused plus the gradient w.r.t. the pose table: v_poses [m,16] = dL/dR (9, row-major) | dL/dt (3) |
 * dL/dq_o2w (4), summed over the rows of each object with radii > 0 (culled rows contribute nothing; an object without
 * rows gets exact zeros; row 0, the background, is computed like the others).  The per-Gaussian outputs are
 * bit-identical to sgn_project_bwd_fused's.  Precondition: object_ids is non-decreasing, and object o owns rows
 * [object_offsets[o], object_offsets[o+1]) (device int32 [m+1], 0 <= offsets <= n) — the layout of
 * sgn_rast.fused.object_ids_for.  Deterministic (per-wave partials in `ws`, then fixed-order sums per object in two
 * small passes; no float atomics).  ws: 16-byte aligned, ws_bytes >= sgn_project_pose_workspace_bytes(n, m) (0 when n < 1 or m < 1).
 * Return codes beyond sgn_project_bwd_fused's: -8 m < 1; -9 object_offsets or v_poses NULL; -10 ws NULL, misaligned
 * or smaller than the workspace size; -11 object_ids and poses both NULL (no pose to differentiate). */
size_t sgn_project_pose_workspace_bytes(int n, int m);
int sgn_project_bwd_fused_pose(int n, const float *means_local, const float *log_scales, float glob_scale,
                               const float *quats_raw, const int32_t *object_ids, const float *poses,
                               const float *viewmat12, float fx, float fy, const float *cov3d,
                               const int32_t *radii, const float *conics, const float *compensation,
                               const float *v_xy, const float *v_depth, const float *v_conic,
                               const float *v_compensation, float *v_means_local, float *v_log_scales,
                               float *v_quats_raw, int semantics, int img_h, int img_w, int m,
                               const int32_t *object_offsets /*device [m+1]*/, float *v_poses /*[m,16]*/, void *ws,
                               size_t ws_bytes, sgn_stream_t stream);

/* Backward of the DROP-IN call `project_gaussians(means, scales, g, X / X.norm(dim=-1, keepdim=True))`
 * (sgn_splatfacto.py:857-873) taken one step further back than sgn_project_bwd: gradients w.r.t. the means, the
 * LOGARITHM of the scales (v_scale * scale — `scales` arrives activated, as the caller computed it, no second exp) and
 * the UN-normalised quaternions X.  Used by the graph proofs of the drop-in operators (sgn_rast/proofs.py) when the
 * autograd graph behind the two arguments shows `torch.exp(...)` and `X / X.norm(...)`; replaces the ~10 small kernels
 * of torch's exp / div / norm backward.  World-frame means, no pose. */
int sgn_project_bwd_act(int n, const float *means3d, const float *scales_activated, float glob_scale,
                        const float *quats_unnormalised, const float *viewmat12, float fx, float fy,
                        const float *cov3d, const int32_t *radii, const float *conics, const float *compensation,
                        const float *v_xy, const float *v_depth, const float *v_conic, const float *v_compensation,
                        float *v_mean3d, float *v_log_scales, float *v_quats_unnormalised, int semantics, int img_h,
                        int img_w, sgn_stream_t stream);

/* Fourier DC fan-out (sgn_splatfacto_scene_graph.py:239-247: an object's effective DC term is
 * `sum(features_dc * idft[..., None], dim=1, keepdim=True)`): for each listed part p, rows [row0[p], row0[p] + rows[p])
 * of v_dc_eff [.,3] become  out_p[r, f, :] = v_dc_eff[row0[p] + r, :] * weights_p[f]  ([rows[p], n_fourier[p], 3]).
 * The four arrays are HOST arrays of length n_parts (weights / out hold device pointers); one launch per 32 parts. */
int sgn_fourier_dc_bwd(int n_parts, const int32_t *row0_host, const int32_t *rows_host, const int32_t *n_fourier_host,
                       const float *const *weights_host, float *const *out_host, const float *v_dc_eff,
                       sgn_stream_t stream);

/* colors = [clamp(. + 0.5, min 0)] SH(degree, means - cam_pos, [dc_eff | features_rest]),
 * dc_eff = sum_f features_dc[:, f, :] * idft[object, f]  (Fourier DC term,
 * sgn_splatfacto_scene_graph.py:239-247,420-433; n_fourier = 1 and idft = {1} for plain models).
 * features_dc [n,n_fourier,3], features_rest [n,k-1,3] (never concatenated), idft [n_objects,n_fourier],
 * cam_pos3 is a device pointer.  The backward needs the forward's `colors` for the clamp mask. */
int sgn_sh_fwd_fused(int n, int k, int degree, const float *means, const float *cam_pos3,
                     const float *features_dc, int n_fourier, const float *features_rest,
                     const int32_t *object_ids, const float *idft, const float *poses /*nullable: means are local*/,
                     int post_half_clamp, float *colors, sgn_stream_t stream);
int sgn_sh_bwd_fused(int n, int k, int degree, const float *means, const float *cam_pos3, int n_fourier,
                     const int32_t *object_ids, const float *idft, const float *poses, int post_half_clamp,
                     const float *colors, const float *v_colors, float *v_features_dc, float *v_features_rest, sgn_stream_t stream);

/* The fused SH front end over UN-CONCATENATED sub-models (round 4; the scene graph keeps one features_dc /
 * features_rest parameter per sub-model: sgn_splatfacto_scene_graph.py:355-360 concatenates them every step, 180 MB each
 * way at 1 M Gaussians).  n_parts <= 32 parts in aggregated order; the four HOST arrays hold, per part: its rows, its
 * Fourier dimension (1..16), device pointers to features_dc [rows, F, 3] and features_rest [rows, k-1, 3].  means /
 * colors / v_colors are the aggregated [N,3] arrays (N = sum of rows); the part index is the object index: pose row
 * (poses [n_parts,16], NULL = no rigid transform) and idft row (idft [n_parts, idft_stride]).  The backward writes each
 * part's gradients into that part's own arrays (v_features_*_host). */
int sgn_sh_fwd_parts(int n_parts, const int32_t *rows_host, const int32_t *n_fourier_host,
                     const float *const *features_dc_host, const float *const *features_rest_host, int k, int degree,
                     const float *means, const float *cam_pos3, const float *idft, int idft_stride, const float *poses,
                     int post_half_clamp, float *colors, sgn_stream_t stream);
int sgn_sh_bwd_parts(int n_parts, const int32_t *rows_host, const int32_t *n_fourier_host, int k, int degree,
                     const float *means, const float *cam_pos3, const float *idft, int idft_stride, const float *poses,
                     int post_half_clamp, const float *colors, const float *v_colors, float *const *v_features_dc_host,
                     float *const *v_features_rest_host, sgn_stream_t stream);

/* Data-parallel SH gradient: v_coeffs[n,k,c] = scale * sum_r basis_k(dir_{r,n}) * v_colors_all[r,n,c]
 * over the n_views ranks' all-gathered colour gradients.  Directions come either from viewdirs_all [R,n,3]
 * (drop-in path) or from means [n,3] (+ optional object_ids/poses) and cam_pos_all [R,3] (fused path); exactly one
 * of the two must be given.  Replaces the dense [n,k,3] all-reduce: 2-4x less traffic on the xGMI links. */
int sgn_sh_bwd_multi(int n, int k, int degree, int n_views, const float *viewdirs_all, const float *means,
                     const float *cam_pos_all, const int32_t *object_ids, const float *poses,
                     const float *v_colors_all, float scale, float *v_coeffs /*[n,k,3]; [n,k-1,3] when v_dc is given*/,
                     float *v_dc /*NULL, or [n,3]: band 0 goes here (the reference keeps features_dc and
                                   features_rest as separate leaves, sgn_splatfacto.py:251-268)*/,
                     sgn_stream_t stream);

/* _C.compute_sh_forward / _C.compute_sh_backward (gsplat/sh.py; reference call sites
 * sgn_splatfacto.py:939, sgn_splatfacto_scene_graph.py:285).  coeffs [n,k,3], k in
 * {1,4,9,16,25}; degree <= 4; directions are normalised inside; no +0.5. */
int sgn_sh_fwd(int n, int k, int degree, const float *viewdirs, const float *coeffs,
               float *colors /*[n,3]*/, sgn_stream_t stream);
int sgn_sh_bwd(int n, int k, int degree, const float *viewdirs, const float *v_colors,
               float *v_coeffs /*[n,k,3], fully written*/, sgn_stream_t stream);

/* torch.cumsum(int32) inside gsplat/utils.py compute_cumulative_intersects. */
size_t sgn_scan_workspace_bytes(int n);
int sgn_scan_i32(int n, const int32_t *in, int32_t *out_inclusive, void *ws, size_t ws_bytes,
                 sgn_stream_t stream);

/* _C.map_gaussian_to_intersects: key = (tile_id << 32) | int32_bits(depth), val = gaussian id,
 * emitted row-major over the tile bbox starting at cum[i-1]. */
int sgn_map_isect(int n, const float *xys, const float *depths, const int32_t *radii,
                  const int32_t *cum_tiles_hit, int tiles_x, int tiles_y, int block_width,
                  int64_t *isect_keys, int32_t *isect_vals, int semantics, sgn_stream_t stream);

/* torch.sort(int64) + gather in gsplat/utils.py bin_and_sort_gaussians: stable LSD radix sort
 * of (key,val) pairs over key bits [begin_bit,end_bit) (keys must be non-negative; bits outside
 * the range must be equal across keys for the result to equal a full 64-bit sort). */
size_t sgn_sort_workspace_bytes(int64_t n_isect);
int sgn_sort_pairs(int64_t n_isect, int begin_bit, int end_bit, const int64_t *keys_in,
                   const int32_t *vals_in, int64_t *keys_out, int32_t *vals_out, void *ws,
                   size_t ws_bytes, int sort_rank_mode, sgn_stream_t stream);

/* `sort_rank_mode` — an ARGUMENT of every sorting entry point (sgn_sort_pairs, sgn_depth_rank, sgn_bin_prepare,
 * sgn_bin_intersect), not library state: which in-wave ranking the scatter pass of the radix sort uses (radix_sort.hip)
 *   0  ballot-match ranking — documented ISA semantics only: THE DEFAULT of the host side;
 *   1  one returning LDS atomic per key — 8x fewer ranking instructions, stable only if same-address lanes of one
 *      ds_add_rtn_u32 are served in ascending lane order (observed on gfx950, not documented).
 * sgn_sort_selftest QUEUES rounds x 16 adversarial probe sorts (all-equal keys, lane-interleaved keys, runs, hashes; both
 * sort-tile sizes) with BOTH rankings on `stream` and ADDS the number of differing output pairs to *mismatches (device
 * int32 the caller zeroed); asynchronous and stateless, so several instances can run on several streams at once.  The
 * host side (sgn_rast/_lib.py) passes 1 only when asked to (SGN_SORT_RANK=atomic) and only on a device where the probe,
 * run under load, counted zero. */
size_t sgn_sort_selftest_workspace_bytes(void);
int sgn_sort_selftest(void *ws, size_t ws_bytes, int rounds, int32_t *mismatches, sgn_stream_t stream);

/* _C.get_tile_bin_edges; tile_bins [n_tiles,2] is zero-filled here first. */
int sgn_tile_bins(int64_t n_isect, const int64_t *keys_sorted, int n_tiles, int32_t *tile_bins,
                  sgn_stream_t stream);

/* Fused binning (what rasterize_gaussians uses internally; same gaussian_ids_sorted / tile_bins as the
 * four upstream-shaped calls above, bit for bit, with ~1/3 of their HBM traffic): the Gaussians are ranked
 * by depth once (stable, ties by id = upstream's emission order), intersections are emitted in rank order,
 * and the list is then stably sorted by tile id only.  Two calls because the host must read
 * n_isect = cum_by_rank[n-1] in between to size the buffers (upstream has the same `.item()` sync in
 * compute_cumulative_intersects). */
size_t sgn_bin_prepare_workspace_bytes(int n);
/* `cull` != 0 (with conics and opacities given): exact tile culling — a (tile, Gaussian) pair is only emitted
 * if some pixel centre of the tile can reach alpha >= 1/255 (the convex set sigma <= ln(255*opacity) + margin meets
 * the tile's pixel-centre rectangle; evaluated per tile row as one interval).  Dropped pairs contribute nothing in forward or backward, so rasterize results
 * are unchanged; the list is then a sub-sequence of upstream's.  With cull == 0 the list equals upstream's. */
/* bin_records [n, SGN_BIN_RECORD_FLOATS] (32 B per Gaussian: centre, conic, alpha-cutoff threshold, radius, kept-tile
 * count) is written by sgn_bin_prepare in id order and read back by sgn_bin_intersect: the rank-order emission
 * gathers one sector per Gaussian instead of five arrays. */
#define SGN_BIN_RECORD_FLOATS 8
int sgn_bin_prepare(int n, const float *xys, const float *depths, const int32_t *radii, const float *conics,
                    const float *opacities, int opacity_is_logit, int cull, int tiles_x, int tiles_y,
                    int block_width, int32_t *cum_by_rank /*[n] inclusive scan of kept-tile counts, rank order*/,
                    int32_t *gid_by_rank /*[n] out; in when rank_ready*/,
                    int rank_ready /*1: gid_by_rank already holds sgn_depth_rank(n, depths, radii, ...)*/,
                    float *bin_records /*[n,8] out*/, void *ws, size_t ws_bytes, int sort_rank_mode,
                    int semantics, sgn_stream_t stream);
/* The first stage of sgn_bin_prepare on its own: gid_by_rank[r] = id of the Gaussian of depth rank r (stable: ties by
 * id; radii <= 0 last).  It reads depths and radii only, so a caller can queue it right behind the projection — before
 * opacities and colours exist — and hand the result to sgn_bin_prepare(rank_ready = 1). */
size_t sgn_depth_rank_workspace_bytes(int n);
int sgn_depth_rank(int n, const float *depths, const int32_t *radii, int32_t *gid_by_rank /*[n]*/, void *ws,
                   size_t ws_bytes, int sort_rank_mode, sgn_stream_t stream);
size_t sgn_bin_intersect_workspace_bytes(int64_t n_isect);
/* n_isect_dev == NULL: n_isect is the intersection count the host has read back (cum_by_rank[n-1]).
 * n_isect_dev != NULL (speculative form, no upstream counterpart): the call is queued BEFORE the host knows the count;
 * n_isect is then the CAPACITY the caller sized gaussian_ids_sorted and the workspace for (e.g. from its previous
 * call) and the kernels read the true count from *n_isect_dev (= cum_by_rank + n - 1) on the device.  If the true
 * count turns out to be <= the capacity the outputs are exactly those of the plain form (rows [0, count) of
 * gaussian_ids_sorted); if it is larger nothing is written out of bounds, the outputs are meaningless and the caller
 * must call again with the real count.  The GPU then works through the emission and the tile sort while the host
 * waits for the count instead of idling through the host's wake-up.
 *
 * quadrant_masks != 0 (16x16 tiles, n < SGN_QMASK_MAX_IDS; no upstream counterpart): every entry of
 * gaussian_ids_sorted carries, in bits 28-31, which of its tile's four 8x8 quadrants the Gaussian can reach with
 * alpha >= 1/255 (bit q: x half = q & 1, y half = q >> 1) — the exact convex test of the culling, evaluated per half
 * band — and the Gaussian id in bits 0-27 (SGN_QMASK_ID_BITS).  The raster kernels then skip quadrants from these bits
 * (sgn_raster_opts.ids_qmask = 1) instead of testing the ellipse's bounding box per entry.  With culling off every
 * entry gets 0xF. */
#define SGN_QMASK_ID_BITS 28
#define SGN_QMASK_MAX_IDS (1 << SGN_QMASK_ID_BITS)
int sgn_bin_intersect(int n, int64_t n_isect, const float *bin_records, const int32_t *cum_by_rank,
                      const int32_t *gid_by_rank, int tiles_x, int tiles_y, int block_width,
                      int32_t *gaussian_ids_sorted /*[n_isect]*/, int32_t *tile_bins /*[tiles,2]*/,
                      int quadrant_masks, void *ws, size_t ws_bytes, const int32_t *n_isect_dev, int sort_rank_mode,
                      sgn_stream_t stream);

/* Sub-list of a binned scene for an id window (no upstream counterpart; the scene graph's objects-only accumulation
 * pass, sgn_splatfacto_scene_graph.py:364-365, served from the main pass's depth list): keeps, in order, the entries of
 * gaussian_ids_sorted whose id (low SGN_QMASK_ID_BITS bits when ids_qmask) lies in [id_lo, id_hi), and writes the bins of
 * the kept list.  ids_out needs room for as many entries as the source list (the kept count stays on the device; the
 * raster kernels read bins only).  Relative order is preserved, so a pass over the sub-list equals the reference's own
 * re-binned pass bit for bit.  ws: sgn_list_window_workspace_bytes(n_tiles). */
size_t sgn_list_window_workspace_bytes(int n_tiles);
int sgn_list_window(int n_tiles, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, int id_lo, int id_hi,
                    int ids_qmask, int32_t *ids_out, int32_t *tile_bins_out /*[n_tiles,2]*/, void *ws, size_t ws_bytes,
                    sgn_stream_t stream);

/* The distinct Gaussian ids a forward pass WALKED (entries [tile_bins[t].x, tile_stats[2t]] of every tile's list:
 * tile_stats is sgn_raster_fwd's per-tile output) — a superset of the rows its backward can give a non-zero gradient,
 * known right after the forward.  The data-parallel row exchange (sgn_rast/dp.py) sends these rows instead of dense
 * gradients.  stamps [n] (int32, zero-filled once, then owned by this call sequence) records the epoch (non-zero, a new
 * value per call) an id was last listed in; list needs n entries; *count receives the number listed.  No upstream
 * counterpart (the reference is single-GPU). */
int sgn_mark_walked(int n_tiles, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const int32_t *tile_stats,
                    int ids_qmask, int epoch, int32_t *stamps, int32_t *list, int32_t *count, sgn_stream_t stream);

/* The two data movements of the data-parallel row exchange (sgn_rast/dp.py; no upstream counterpart).
 * sgn_rows_pack: message = [header row | count rows] of row_words floats each; header = header3 (3 floats) + zeros;
 * row i = [bits of id = list[i] | rows id of the n_tensors (<= 8) per-Gaussian float tensors side by side (widths_host[j]
 * floats each; a NULL source contributes zeros)].  srcs_host / widths_host are HOST arrays (device pointers inside).
 * sgn_rows_scatter: the rows of ONE rank's message added (x scale) into the dense per-tensor sums dsts_host[j][id]; the
 * last tail_words floats of each row are copied to tail_out[id] (may be NULL with tail_words 0 ... and are NOT scaled).
 * Ids are unique within a message; call once per rank, in rank order, for replica-identical sums. */
int sgn_rows_pack(int count, const int32_t *list, int n_tensors, const float *const *srcs_host,
                  const int32_t *widths_host, const float *header3, float *out, int row_words, sgn_stream_t stream);
int sgn_rows_scatter(int count, const float *rows /*incl. header row*/, int row_words, int n_tensors,
                     float *const *dsts_host, const int32_t *widths_host, float scale, int tail_words, float *tail_out,
                     sgn_stream_t stream);
/* Contract check of the row exchange: *count = rows of the n_tensors per-Gaussian gradient tensors (NULL = no gradient)
 * that hold a non-zero word although sgn_mark_walked did not list their id in `epoch` (stamps[id] != epoch) — rows the
 * exchange would not send (a regulariser on per-Gaussian parameters, any loss term beside the rendered images). */
int sgn_rows_outside(int n, int n_tensors, const float *const *srcs_host, const int32_t *widths_host,
                     const int32_t *stamps, int epoch, int32_t *count, sgn_stream_t stream);

/* Window recognition for the drop-in scene-graph path (no upstream counterpart).  The reference renders its sub-model
 * passes (sgn_splatfacto_scene_graph.py:364-366) from torch.cat COPIES of per-model slices of the main projection
 * (:270-276).  mismatch[c] (device, int32, c < n_cand <= 4) becomes 0 iff the window tensors equal rows
 * [cand_lo_host[c], cand_lo_host[c] + n_win) of the full-scene tensors BIT FOR BIT (xys [.,2], depths, radii,
 * num_tiles_hit; conics [.,3] and opacities too when given - the exact tile culling depends on them); the caller may
 * then rasterize the window over the depth list binned for the full scene (sgn_raster_fwd with id range + window).
 * Any tensor pair may be omitted (NULL on BOTH sides) when the caller has settled it another way — the Python host
 * proves the four differentiable tensors from the autograd graph and sends only radii / num_tiles_hit. */
int sgn_rows_match(int n_win, int n_full, int n_cand, const int32_t *cand_lo_host, const float *xys_w,
                   const float *depths_w, const int32_t *radii_w, const int32_t *num_tiles_hit_w, const float *conics_w,
                   const float *opacities_w, const float *xys, const float *depths, const int32_t *radii,
                   const int32_t *num_tiles_hit, const float *conics, const float *opacities, int32_t *mismatch,
                   sgn_stream_t stream);

/* Launch order for the raster kernels (no upstream counterpart): order[0..n_tiles) = the tiles sorted by length,
 * longest class first (half-octave classes); order[n_tiles] = n_long, the number of leading entries whose class is at
 * least that of `long_thresh` (0 when long_thresh <= 0).  "Length" is the depth-list length of tile_bins, or - with
 * tile_stats (sgn_raster_fwd's output) - the reverse-walk length the backward will see; with small_q16 > 0 a tile whose
 * forward evaluated fewer than small_q16 / 16 (entry, quadrant) pairs per walked entry (small splats) counts as long.
 * Results do not depend on the order; on skewed content it removes the tail of late-starting long tiles, and n_long
 * drives the backward's two-kernel adaptive scheme (sgn_raster_bwd).  `order` has n_tiles + 2 entries; the last one is
 * 0, or - with tile_stats, images of up to 16384 tiles - 1000 * (list entries the forward WALKED before its tiles
 * saturated) / (entries listed): the statistic the host's quadrant-mask policy reads back (sgn_bin_intersect).
 * scratch (sgn_tile_order_scratch_bytes(n_tiles); int32 words, ZERO-FILLED before its first use, left zero-filled by
 * every call, one per stream: calls that share it must be stream-ordered) selects the multi-workgroup form (any tile
 * count below 2^26, the statistic included); NULL keeps the single-workgroup kernels. */
size_t sgn_tile_order_scratch_bytes(int n_tiles);
int sgn_tile_order(int n_tiles, const int32_t *tile_bins, const int32_t *tile_stats, int long_thresh, int small_q16,
                   int32_t *order, void *scratch, size_t scratch_bytes, sgn_stream_t stream);

/* _C.rasterize_forward (3-channel path; reference call sites sgn_splatfacto.py:954-967,
 * :982-994).  `recs_ws` (>= sgn_raster_workspace_bytes(n, n_isect, opts): one 48-byte row per Gaussian) receives the
 * rows the kernels read through the scalar cache; keep it alive and pass recs_packed=1 to sgn_raster_bwd to skip
 * rebuilding them. */
size_t sgn_raster_workspace_bytes(int n, int64_t n_isect, const sgn_raster_opts *opts);
int sgn_raster_fwd(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                   const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                   const float *conics, const float *colors /*[n,3]*/, const float *opacities /*[n]*/,
                   int opacity_is_logit /*0 = gsplat semantics; 1 = fuse torch.sigmoid (sgn_splatfacto.py:949)*/,
                   int id_lo, int id_hi /*only Gaussians with id in [id_lo, id_hi) take part (0, n = all): a sub-model
                                          pass of the scene graph (sgn_splatfacto_scene_graph.py:364-366) over the
                                          depth list binned once for the whole scene*/,
                   int window /*1: xys / conics / colors / opacities hold rows [id_lo, id_hi) ONLY (row g - id_lo): the
                                sub-model's own tensors, while gaussian_ids_sorted / tile_bins index all n Gaussians of
                                the scene the list was binned for (the drop-in scene-graph path: the caller hands
                                torch.cat COPIES of per-model slices, recognised by content)*/,
                   const float *background3, float *out_img /*[H,W,3]*/, float *final_Ts /*[H,W]*/,
                   int32_t *final_idx /*[H,W]*/, void *recs_ws, size_t recs_ws_bytes,
                   int rows_built /*1: sgn_raster_build_rows already filled recs_ws*/,
                   const int32_t *tile_order /*NULL, or sgn_tile_order's permutation of the tiles: launch order*/,
                   int32_t *tile_stats /*NULL, or [tiles,2] out: deepest list position composited by any pixel of the tile;
                                         number of (entry, quadrant) pairs evaluated*/,
                   const float *depths /*NULL, or [n] (the projection's depths): also accumulate the DEPTH CHANNEL
                                         out_depth[p] = sum_g depths[g] * alpha_g * T_g — what the reference obtains from a
                                         second rasterization of depths.repeat(1, 3) with a zero background
                                         (sgn_splatfacto.py:982-994), for one fma per evaluated pair; not with window = 1*/,
                   float *out_depth /*[H,W]; with depths*/,
                   const int32_t *skip_flag /*NULL, or a device int: when it reads 0 every kernel of this call returns at
                                              once (the caller answers the pass with sgn_depth_reuse); needs
                                              rows_built = 1*/,
                   const sgn_raster_opts *opts, sgn_stream_t stream);
/* sgn_raster_fwd with TWO GROUP ACCUMULATIONS riding on the same walk (no upstream counterpart): besides everything
 * sgn_raster_fwd writes, the final transmittance / final index / per-tile walk depth of the pass that would render only
 * the Gaussians with id < split ("head") and of the pass that would render only those with id >= split ("tail") over
 * the same depth list — the scene graph's background-only and objects-only accumulation passes
 * (sgn_splatfacto_scene_graph.py:364-366), for which the reference rasterizes twice more.  Every entry belongs to one
 * group, its alpha is the one the main pass evaluates anyway; per entry the group costs one more transmittance
 * recursion with the single pass's arithmetic, so the group state is BIT-EQUAL to what sgn_raster_fwd calls with id
 * ranges [0, split) / [split, n) write as final_Ts / final_idx / tile_stats[:, 0] (tests/test_gpu_groups.py); a group's
 * backward is sgn_raster_bwd with that id range, v_out_img = NULL and the group's state.
 *   group_state [4][H*W]: T_head, T_tail (float), then final index head, tail (int32);
 *   group_stats [2][tiles*2]: like tile_stats, head then tail.
 * ONE group (own_group: 0 head, 1 tail, -1 none) may come with its own compacted list (own_ids / own_bins from
 * sgn_list_window — the list its backward will walk): its indices are then positions of THAT list, and when it is still
 * alive after the main pass and the other group have finished (a few objects in front of a saturated background) it
 * goes on along its own list instead of dragging the shared walk to the end.  The other group's indices are positions
 * of the shared list.  Packed forward only (16x16 tiles; the whole scene): -12 otherwise. */
int sgn_raster_fwd_groups(int img_h, int img_w, int n, int64_t n_isect, const int32_t *gaussian_ids_sorted,
                          const int32_t *tile_bins, const float *xys, const float *conics, const float *colors,
                          const float *opacities, int opacity_is_logit, const float *background3, float *out_img,
                          float *final_Ts, int32_t *final_idx, void *recs_ws, size_t recs_ws_bytes, int rows_built,
                          const int32_t *tile_order, int32_t *tile_stats, const float *depths, float *out_depth,
                          int split, int own_group, const int32_t *own_ids, const int32_t *own_bins /*[tiles,2]*/,
                          float *group_state, int32_t *group_stats, const sgn_raster_opts *opts, sgn_stream_t stream);
/* The LAYERED forward of evaluation renders (no upstream counterpart; forward only): ONE walk of the depth list
 * composites three layers per pixel — "all" (every entry; colour, the depth channel, T), "head" (ids < split: the scene
 * graph's background sub-model; colour, T) and "tail" (ids >= split: the objects; colour, T) — where the reference
 * rasterizes six times (sgn_splatfacto.py:954-994 for the scene, sgn_splatfacto_scene_graph.py:364-372 for the two
 * sub-model accumulations and, in eval mode, the two sub-model images).  An entry's alpha is evaluated once; each layer it
 * belongs to runs the single pass's recursion on its own state, in the single pass's operation order, so a layer's image
 * and final transmittance are BIT-EQUAL to sgn_raster_fwd over that id range, in both exact_exp modes
 * (tests/test_gpu_layers.py).  Rows, sorted ids (quadrant masks included: opts->ids_qmask), bins and tile order are the
 * ones sgn_raster_fwd takes; the binning is done once for the whole scene.
 *   out_img  [3][H,W,3]  C + T * background of all / head / tail      final_Ts [3][H,W]      out_depth [H,W] (all)
 * own_ids / own_bins (both or neither): the tail layer's own compacted list from sgn_list_window(split, n).  With it the
 * shared walk ends when the all-layer and the head layer are finished and the tail layer goes on along its own list (a few
 * objects in front of a saturated background never finish); tiles without a tail entry run a one-layer walk.  An empty
 * layer (split == 0 or split == n) comes back as T = 1, image = background.
 * 16x16 tiles only: block_width != 16 returns -12. */
int sgn_raster_layers_fwd(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                          const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                          const float *conics, const float *colors, const float *opacities, int opacity_is_logit,
                          const float *background3, const float *depths, int split, const int32_t *own_ids,
                          const int32_t *own_bins /*[tiles,2]*/, float *out_img, float *final_Ts, float *out_depth,
                          void *recs_ws, size_t recs_ws_bytes, int rows_built, const int32_t *tile_order,
                          const sgn_raster_opts *opts, sgn_stream_t stream);
/* The per-pixel finish of an evaluation render over the three layers of sgn_raster_layers_fwd, one launch, in the
 * reference's operation order (sgn_splatfacto.py:968-996 with self.training == False; no fma is formed, so every output
 * equals the eager torch expression bit for bit):
 *   acc[l] = 1 - T[l];   rgb[l] = clamp(clamp(img[l], max=1) * acc[l] + sky * (1 - acc[l]), 0, 1) for all and head,
 *   rgb[tail] = clamp(clamp(img[tail], max=1), 0, 1) (scene_graph.py:371 passes no sky);   depth = acc[all] > 1e-3 ?
 *   D / acc[all] : 10.   sky [H,W,3] may be NULL (use_sky_sphere = False): no blend on any layer.
 *   rgb [3][H,W,3], acc [3][H,W], depth [H,W]. */
int sgn_layers_finish(int img_h, int img_w, const float *layer_img, const float *layer_Ts, const float *depth_channel,
                      const float *sky, float *rgb, float *acc, float *depth, sgn_stream_t stream);
/* The FEATURE rasterizer (csrc/raster_features.hip; upstream's counterpart is the N-D path of rasterize_gaussians, which
 * the reference never takes): alpha-composites n_channels (K, 1..64) arbitrary per-Gaussian values features [n,K] over an
 * existing depth list — class logits, the projection's depths, object ids — evaluating each (pixel, Gaussian) alpha once
 * per chunk of up to 16 channels (K <= 16: one walk of the lists; K <= 64: ceil(K / 16) walks inside the one call), where
 * the 3-channel entries need ceil(K / 3) passes.  The per-entry arithmetic is the contract of sgn_raster_fwd (header of
 * csrc/raster.hip), operation for operation, so every channel of out_img, final_Ts and final_idx are BIT-EQUAL to a
 * 3-channel pass that carries that channel, in both exact_exp modes (tests/test_gpu_features.py).
 *   out_img [H,W,K] = F + T * background      final_Ts [H,W]      final_idx [H,W]
 * List, bins, xys, conics, opacities, opacity_is_logit (0 / 1), opts (exact_exp and ids_qmask are read; NULL = defaults)
 * and stream mean what they mean to sgn_raster_fwd.  Whole scene only: no id range, no window, no launch order.
 * background [K] may be NULL (zeros, the natural background of features).  ws >=
 * sgn_raster_features_workspace_bytes(n) receives the per-Gaussian geometry rows; nothing in it has to survive the call.
 * n_isect == 0: the list pointers, the per-Gaussian arrays and ws may be NULL; out_img = background, final_Ts = 1,
 * final_idx = 0.
 * Errors (checked in this order, before any launch): -12 block_width != 16; -1 image size / n; -13 n_channels outside
 * 1..64; -3 n_isect; -4 a NULL output; -5 a NULL input (n_isect > 0); -6 ws too small; -11 ids_qmask with n >= 2^28. */
size_t sgn_raster_features_workspace_bytes(int n);
int sgn_raster_features_fwd(int img_h, int img_w, int block_width, int n, int n_channels, int64_t n_isect,
                            const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                            const float *conics, const float *features /*[n,K]*/, const float *opacities /*[n]*/,
                            int opacity_is_logit, const float *background /*[K] or NULL*/, float *out_img /*[H,W,K]*/,
                            float *final_Ts /*[H,W]*/, int32_t *final_idx /*[H,W]*/, void *ws, size_t ws_bytes,
                            const sgn_raster_opts *opts, sgn_stream_t stream);
/* Its backward: the reverse per-pixel walk from final_idx with the recursion, the operation order (ra = rcp(1 - alpha),
 * the T recursion, the v_sigma chain) and the alpha_clamp_bwd handling of sgn_raster_bwd, the chunks' geometry gradients
 * added into the same per-Gaussian sums (v_alpha is linear in the channels).  v_out_img [H,W,K] and v_out_alpha [H,W] may
 * each be NULL (zeros).  Outputs, every row written (zero where the Gaussian touched nothing): v_xy [n,2], v_conic [n,3]
 * ([:,1] is the TRUE derivative, as sgn_raster_bwd's: sgn_project_bwd takes it as is), v_features [n,K], v_opacity [n]
 * (w.r.t. the probability with opacity_is_logit = 0, w.r.t. the logit with 1).  ws as in the forward (the rows are
 * rebuilt; the per-Gaussian sums live behind them).  reduce_mode and debug_flags of opts are not read: there is one
 * reduction, the transposed one.  n == 0 returns 0 at once; n_isect == 0 writes zeros.
 * Errors: the forward's codes, and -4 also for a NULL gradient output / conics / opacities / ws, -5 a NULL list or state
 * input (n_isect > 0), -7 alpha_clamp_bwd outside (0, 1). */
int sgn_raster_features_bwd(int img_h, int img_w, int block_width, int n, int n_channels, int64_t n_isect,
                            const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                            const float *conics, const float *features, const float *opacities, int opacity_is_logit,
                            const float *background, const float *final_Ts, const int32_t *final_idx,
                            const float *v_out_img, const float *v_out_alpha, float alpha_clamp_bwd, float *v_xy,
                            float *v_conic, float *v_features, float *v_opacity, void *ws, size_t ws_bytes,
                            const sgn_raster_opts *opts, sgn_stream_t stream);
/* Softmax cross-entropy of a logit image against a uint8 label map (csrc/semantic_loss.hip; the semantic term of the
 * Street Gaussians paper; torch.nn.functional.cross_entropy(logits.view(-1, K), labels.view(-1).long(), ignore_index)
 * with reduction = "mean"):  loss_out[0] = mean over COUNTED pixels of logsumexp(logits[p]) - logits[p, labels[p]].
 * A pixel counts when labels[p] != ignore_index (-1: none), labels[p] < n_classes and — with mask [H,W] bytes, NULL = no
 * mask — mask[p] != 0.  The sum (fp64) and the count are reduced on the device into ws (>=
 * sgn_semantic_ce_workspace_bytes(), 16 bytes), loss_out is DEVICE memory: no host read-back.  No counted pixel: loss 0.
 * The backward takes the forward's ws (the count) and v_loss (DEVICE, one float) and writes v_logits [H,W,K] =
 * (softmax - onehot) * v_loss / count, zero on every pixel that does not count (so all zeros, no NaN, when none does).
 * Errors: -1 image size; -2 n_classes outside 1..64; -3 ignore_index outside -1..255; -4 a NULL pointer (mask may be
 * NULL); -5 ws too small. */
size_t sgn_semantic_ce_workspace_bytes(void);
int sgn_semantic_ce_fwd(int img_h, int img_w, int n_classes, const float *logits /*[H,W,K]*/,
                        const unsigned char *labels /*[H,W]*/, int ignore_index, const unsigned char *mask,
                        float *loss_out /*device [1]*/, void *ws, size_t ws_bytes, sgn_stream_t stream);
int sgn_semantic_ce_bwd(int img_h, int img_w, int n_classes, const float *logits, const unsigned char *labels,
                        int ignore_index, const unsigned char *mask, const float *v_loss /*device [1]*/, const void *ws,
                        size_t ws_bytes, float *v_logits /*[H,W,K]*/, sgn_stream_t stream);
/* ONE call per autograd node (round 5; no upstream counterpart: upstream's rasterize_gaussians drives its five `_C`
 * calls from Python).  The whole forward of `rasterize_gaussians` over the full scene: sgn_bin_prepare ->
 * asynchronous read-back of the intersection count -> sgn_raster_build_rows -> SPECULATIVE sgn_bin_intersect (sized by
 * isect_capacity, the true count read on the device) -> wait for the count (the path's one host sync, upstream's
 * `.item()`) -> sgn_tile_order -> sgn_raster_fwd, all on `stream`, temporaries carved from ONE caller-provided arena
 * (sgn_rasterize_arena_bytes).  The outputs the node keeps for its backward are the caller's: gaussian_ids_sorted
 * [isect_capacity], tile_bins [tiles,2], tile_order [tiles+2], tile_stats [tiles,2], rows (sgn_raster_workspace_bytes(n,
 * 0, opts)), final_Ts, final_idx.  *n_isect_host receives the true count.  Returns 0; SGN_E_CAPACITY when the count
 * exceeds isect_capacity (nothing rasterized: call again with more room); with a count of 0 it returns 0 without touching
 * out_img / final_Ts / final_idx (tile_bins is zero-filled): the caller writes the background image.
 * gid_by_rank_ready: NULL, or sgn_depth_rank's result for these depths / radii (started earlier).  count_pinned: pinned
 * host int32 the count arrives in (NULL: a pageable copy) — written by the scan kernel itself where the word is mapped into
 * the device's address space (hipHostMalloc'd memory is: no copy command and — round 6 — no event on the stream; the
 * host polls the word, poisoned with -1 before the launch), copied otherwise.  extra_dev / extra_pinned: one more
 * device int32 to bring along (the host's walk statistic), or NULL: stored by the same thread ahead of the count.  order_scratch as in sgn_tile_order. */
#define SGN_E_CAPACITY (-100)
size_t sgn_rasterize_arena_bytes(int n, int64_t isect_capacity);
int sgn_rasterize_fwd_all(int n, const float *xys, const float *depths, const int32_t *radii, const float *conics,
                          const float *colors, const float *opacities, int opacity_is_logit, int cull, int img_h,
                          int img_w, int block_width, const float *background3, const int32_t *gid_by_rank_ready,
                          int quadrant_masks, float *out_img, float *final_Ts, int32_t *final_idx,
                          float *out_depth /*NULL, or [H,W]: also accumulate the depth channel (sgn_raster_fwd)*/,
                          int32_t *gaussian_ids_sorted, int64_t isect_capacity, int32_t *tile_bins,
                          int32_t *tile_order, int32_t *tile_stats, void *rows, size_t rows_bytes,
                          void *order_scratch, size_t order_scratch_bytes, void *arena, size_t arena_bytes,
                          int32_t *count_pinned, const int32_t *extra_dev, int32_t *extra_pinned,
                          int64_t *n_isect_host, int sort_rank_mode, int semantics, const sgn_raster_opts *opts,
                          sgn_stream_t stream);

/* ONE call for a sub-model pass over a CACHED list (round 6; no upstream counterpart).  The scene graph renders its
 * objects-only / background-only accumulation passes (sgn_splatfacto_scene_graph.py:364-366) from torch.cat COPIES of
 * per-model slices of the main projection: the call's tensors (`*_w`, n_win rows) are then a row window of the scene
 * (n_full rows) the cached list (gaussian_ids_sorted [n_isect], tile_bins) was binned for.  The call queues the
 * comparison that proves it (sgn_rows_match over every tensor pair whose full-scene side is non-NULL, at the n_cand <= 4
 * candidate offsets cand_lo_host), reads its verdict back (verdict_pinned: pinned host int32[8] or NULL; [0, 4) the
 * verdicts, [7] the word a one-wave kernel behind the comparison stores 1 into and the host polls — this path's one
 * host sync, in place of the intersection-count read-back of the binning it saves), and on a match queues the window's
 * rows (sgn_raster_build_rows, window form), — sub_list != 0 — its compacted sub-list (sgn_list_window into ids_out
 * [n_isect] / tile_bins_out), the launch order (tile_order [tiles + 2] out, unless tile_order_ready hands in the shared
 * list's and no sub-list is made) and sgn_raster_fwd(window = 1).  *matched_lo_host = the matching row offset, or -1:
 * nothing matched and nothing was rasterized (the caller bins the tensors as a scene of their own).  With every
 * full-scene pointer NULL nothing is compared and cand_lo_host[0] is taken as settled by the caller.  The node keeps
 * ids_out / tile_bins_out (or the shared list), tile_order, tile_stats [tiles,2], rows (sgn_raster_workspace_bytes(n_full,
 * 0, opts)), final_Ts, final_idx for its backward.  arena: sgn_rasterize_window_arena_bytes(tiles). */
size_t sgn_rasterize_window_arena_bytes(int n_tiles);
int sgn_rasterize_window_all(int n_win, int n_full, int n_cand, const int32_t *cand_lo_host, const float *xys_w,
                             const float *depths_w, const int32_t *radii_w, const int32_t *num_tiles_hit_w,
                             const float *conics_w, const float *colors_w, const float *opacities_w,
                             int opacity_is_logit, const float *xys, const float *depths, const int32_t *radii,
                             const int32_t *num_tiles_hit, const float *conics, const float *opacities,
                             int64_t n_isect, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                             int ids_qmask, int img_h, int img_w, int block_width, const float *background3,
                             int sub_list, const int32_t *tile_order_ready, float *out_img, float *final_Ts,
                             int32_t *final_idx, int32_t *ids_out, int32_t *tile_bins_out, int32_t *tile_order,
                             int32_t *tile_stats, void *rows, size_t rows_bytes, void *order_scratch,
                             size_t order_scratch_bytes, void *arena, size_t arena_bytes, int32_t *verdict_pinned,
                             int *matched_lo_host /*host*/, const sgn_raster_opts *opts, sgn_stream_t stream);

/* The 48-byte per-Gaussian rows the raster kernels read do not depend on the intersection list: they can be built
 * while the host waits for the intersection count (keeps the GPU busy across that sync); pass rows_built = 1 to
 * sgn_raster_fwd then. */
int sgn_raster_build_rows(int n, const float *xys, const float *conics, const float *colors, const float *opacities,
                          int opacity_is_logit, int id_lo, int id_hi, int window, void *recs_ws, size_t recs_ws_bytes,
                          const int32_t *skip_flag /*as in sgn_raster_fwd*/, sgn_stream_t stream);

/* Answering the reference's depth pass from the first pass's depth channel, without a host sync (no upstream
 * counterpart).  The second rasterize_gaussians call of a step (sgn_splatfacto.py:982-994) has the first call's
 * geometry and `depths[:, None].repeat(1, 3)` as colours.  sgn_colors_match_depths sets *flag = 0 iff colors[i, c] ==
 * depths[i] bit for bit for all i, c (1 otherwise); the caller queues the ordinary forward with skip_flag = flag and
 * then sgn_depth_reuse, which — iff *flag == 0 — writes out_img[p, c] = fma(final_T[p], background[c], depth[p])
 * (the very expression the rasterization ends with) and copies the first pass's final_Ts / final_idx into the second
 * pass's own buffers (its backward reads them).  flag == NULL: unconditional (a caller that can PROVE the colours are
 * the depths on the host — e.g. on the autograd graph — skips the comparison and the conditional forward altogether);
 * final_Ts == final_idx == NULL: no copies (the caller lets the second pass share the first pass's buffers).
 * Bit-equal to the two-pass result in exact-exp mode. */
int sgn_colors_match_depths(int n, const float *colors /*[n,3]*/, const float *depths /*[n]*/, int32_t *flag,
                            sgn_stream_t stream);
int sgn_depth_reuse(int img_h, int img_w, const int32_t *flag, const float *depth_channel /*[H,W]*/,
                    const float *final_Ts_first, const int32_t *final_idx_first, const float *background3,
                    float *out_img /*[H,W,3]*/, float *final_Ts, int32_t *final_idx,
                    int n_stats /*0, or 2 * tiles: also copy the first pass's tile statistics*/,
                    const int32_t *tile_stats_first, int32_t *tile_stats, sgn_stream_t stream);

/* _C.rasterize_backward.  alpha_clamp_bwd: 0.99f reproduces gsplat 0.1.x (which clamps at
 * 0.999 in forward and 0.99 in backward).  Outputs are fully written (zero-filled first).
 * v_conic[:,1] is the TRUE derivative dL/d(conic.y) (sum of v_sigma dx dy: what autograd through gsplat's
 * _torch_impl gives); sgn_project_bwd spreads v_conic.y / 2 over the two off-diagonal slots of the symmetric
 * matrix gradient.  (Rounds 1-2 carried half of it here with the un-halved matrix: same end-to-end gradients.)
 * opacity_is_logit: 0 = `opacities` are probabilities, v_opacity is w.r.t. them (upstream); 1 = they are logits, the
 * kernels apply the sigmoid and v_opacity is w.r.t. the logits (fused API); 2 = they are probabilities that the caller
 * obtained as sigmoid(logits) (sgn_splatfacto.py:949) and v_opacity is wanted w.r.t. those logits: v * o * (1 - o). */
size_t sgn_raster_bwd_workspace_bytes(int n);
int sgn_raster_bwd(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                   const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                   const float *conics, const float *colors, const float *opacities, int opacity_is_logit,
                   int id_lo, int id_hi, int window /*as in sgn_raster_fwd; the four outputs then have id_hi - id_lo rows*/,
                   const float *background3, const float *final_Ts, const int32_t *final_idx,
                   const float *v_out_img /*[H,W,3]; NULL = zeros (only alpha reached the loss)*/, const float *v_out_alpha /*[H,W]*/,
                   float alpha_clamp_bwd, float *v_xy /*[n,2]*/, float *v_conic /*[n,3]*/,
                   float *v_colors /*[n,3]*/, float *v_opacity /*[n]*/, void *recs_ws,
                   size_t recs_ws_bytes, int recs_packed, void *grad_ws, size_t grad_ws_bytes,
                   const int32_t *tile_order /*NULL, or sgn_tile_order(..., tile_stats, opts->adapt_bwd, ...): its
                                               first n_long tiles (walks >= adapt_bwd) run four
                                               lean waves per tile, persistent and longest first, the rest one wave per
                                               tile; NULL = in-kernel split of long walks*/,
                   const float *colors_pre_clamp /*NULL, or [n,3] (window: [id_hi - id_lo, 3]): the caller's colours were
                                                   clamp(pre, min = 0) of this tensor (sgn_splatfacto.py:940) and
                                                   v_colors is wanted w.r.t. `pre`: zero where pre < 0*/,
                   const sgn_raster_opts *opts, sgn_stream_t stream,
                   sgn_stream_t aux_stream /*NULL, or a second stream of the same device: the two halves of the
                                             adaptive scheme touch disjoint tiles and then run concurrently (forked
                                             behind `stream`'s queue, joined before the gradients are unpacked)*/);

/* One of SEVERAL reverse walks whose gradients belong to the same tensors (the main pass of sgn_raster_fwd_groups and
 * the group accumulations that reached the loss): all of them accumulate into ONE packed gradient workspace and the last
 * one unpacks — instead of a 48 MB clear, an unpack and four tensor additions per extra walk.  Arguments as
 * sgn_raster_bwd; first != 0 clears grad_ws, last != 0 unpacks it (only then are v_xy / v_conic / v_colors / v_opacity
 * written).  Whole-tensor passes only (window = 0), all with the same conics / opacities / opacity_is_logit; -13
 * otherwise. */
int sgn_raster_bwd_part(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                        const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                        const float *conics, const float *colors, const float *opacities, int opacity_is_logit,
                        int id_lo, int id_hi, int window, const float *background3, const float *final_Ts,
                        const int32_t *final_idx, const float *v_out_img, const float *v_out_alpha,
                        float alpha_clamp_bwd, float *v_xy, float *v_conic, float *v_colors, float *v_opacity,
                        void *recs_ws, size_t recs_ws_bytes, int recs_packed, void *grad_ws, size_t grad_ws_bytes,
                        const int32_t *tile_order, const float *colors_pre_clamp, const sgn_raster_opts *opts,
                        sgn_stream_t stream, sgn_stream_t aux_stream, int first, int last);

/* sgn_raster_bwd_part with the ABSGRAD statistic (AbsGS; gsplat's `absgrad=True` / `means2d.absgrad`; no gsplat 0.1.x
 * counterpart): besides the signed gradients, v_xy_abs [n,2] = per Gaussian the sum over the pixels its reverse walk
 * composites it onto of the ABSOLUTE per-pixel screen-space gradient,
 *     v_xy_abs[g] = sum_pixels ( |A p + B q|, |B p + C q| ),   (p, q) = v_sigma * (dx, dy),  (A, B, C) = conic[g]
 * where the signed v_xy[g] is the same sum without the bars (so v_xy_abs >= |v_xy| up to rounding).  Densification that
 * thresholds the norm of v_xy misses large splats over fine texture, whose per-pixel terms cancel; this does not.  fp32
 * contract per evaluated (pixel, entry) pair: ax += fabsf(fmaf(A, p, B * q)), ay += fabsf(fmaf(B, p, C * q)), no
 * contraction; the sums over a tile's pixels are a wave reduction and the sums over tiles float atomics, as for the
 * signed gradients.  The signed outputs are those of sgn_raster_bwd_part (same body, same arithmetic, same order).
 * Arguments as sgn_raster_bwd_part; window != 0 is an argument error (-13) and so is v_xy_abs == NULL (-14).
 * The two sums live in slots 9 and 10 of a Gaussian's row of the packed gradient workspace (12 floats; the plain walks
 * use slots 0-8 and leave the rest as the clear left them).  When several walks chain into one workspace (first / last),
 * ONLY the walks issued through this entry add to slots 9 and 10 — a group-accumulation walk issued through
 * sgn_raster_bwd_part contributes to the signed gradients alone — and the LAST walk must go through this entry for
 * v_xy_abs (and the other four outputs) to be written: sgn_raster_bwd_part's unpack does not read those slots.  n == 0:
 * nothing is written; n_isect == 0 with last != 0: zeros. */
int sgn_raster_bwd_abs(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                       const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                       const float *conics, const float *colors, const float *opacities, int opacity_is_logit,
                       int id_lo, int id_hi, int window, const float *background3, const float *final_Ts,
                       const int32_t *final_idx, const float *v_out_img, const float *v_out_alpha,
                       float alpha_clamp_bwd, float *v_xy, float *v_conic, float *v_colors, float *v_opacity,
                       void *recs_ws, size_t recs_ws_bytes, int recs_packed, void *grad_ws, size_t grad_ws_bytes,
                       const int32_t *tile_order, const float *colors_pre_clamp, const sgn_raster_opts *opts,
                       sgn_stream_t stream, sgn_stream_t aux_stream, int first, int last, float *v_xy_abs /*[n,2]*/);

/* The backward of a rasterize node as ONE call (round 6): sgn_tile_order over the forward's tile statistics (tile_order
 * [tiles + 2] out — NULL: no reordering, the in-kernel split of long walks —, long walks = opts->adapt_bwd, the
 * small-splat promotion small_q16 only when stats_have_pairs) + sgn_raster_bwd (first = last = 1; window allowed) or
 * sgn_raster_bwd_part (otherwise).  Everything else as in sgn_raster_bwd. */
int sgn_rasterize_bwd_all(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                          const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const int32_t *tile_stats,
                          int stats_have_pairs, const float *xys, const float *conics, const float *colors,
                          const float *opacities, int opacity_is_logit, int id_lo, int id_hi, int window,
                          const float *background3, const float *final_Ts, const int32_t *final_idx,
                          const float *v_out_img, const float *v_out_alpha, float alpha_clamp_bwd, float *v_xy,
                          float *v_conic, float *v_colors, float *v_opacity, void *recs_ws, size_t recs_ws_bytes,
                          int recs_packed, void *grad_ws, size_t grad_ws_bytes, int32_t *tile_order,
                          void *order_scratch, size_t order_scratch_bytes, int small_q16,
                          const float *colors_pre_clamp, const sgn_raster_opts *opts, sgn_stream_t stream,
                          sgn_stream_t aux_stream, int first, int last);

/* pytorch3d.transforms.quaternion_multiply as object2world_gs uses it (sgn_splatfacto_scene_graph.py:416): Hamilton
 * product a (x) b, real part first, result standardised to a non-negative real part.  `a` is EITHER one quaternion
 * for all rows, passed as a HOST array of 4 floats (a_host4; the reference's quat_o2w is a CPU tensor), OR one per row
 * (a_rows, device [n,4]); exactly one of the two is non-NULL.  b, out, v_out, v_b: device [n,4], 16-byte aligned.
 * Backward: v_b (may be NULL) and, for per-row a only, v_a_rows (may be NULL). */
int sgn_quat_mul_fwd(int n, const float *a_host4, const float *a_rows, const float *b, float *out, sgn_stream_t stream);
int sgn_quat_mul_bwd(int n, const float *a_host4, const float *a_rows, const float *b, const float *v_out, float *v_b,
                     float *v_a_rows, sgn_stream_t stream);

/* Sky cube-map lookup: replaces nvdiffrast `dr.texture(tex[None], dirs, filter_mode='linear',
 * boundary_mode='cube')` used by EnvLight (sgn_splatfacto.py:109-150).  tex [6,R,R,C] (faces +x,-x,+y,-y,+z,-z),
 * dirs [h,w,3] (the [H,W] grid of uv; need not be normalised; use h = 1 for a flat list), out [h,w,C];
 * resolution <= 16384.  The backward works in 16x16 tiles of that grid (neighbouring pixels share texels).  The backward returns the texture gradient only (the directions
 * come from the camera and carry no gradient in the reference) and zero-fills v_tex first. */
int sgn_cube_texture_fwd(int h, int w, int resolution, int channels, const float *tex, const float *dirs,
                         float *out, sgn_stream_t stream);
int sgn_cube_texture_bwd(int h, int w, int resolution, int channels, const float *dirs, const float *v_out,
                         float *v_tex, sgn_stream_t stream);

/* Fused EnvLight.forward (sgn_splatfacto.py:117-150): per-pixel camera ray -> world (c2w: DEVICE pointer to a
 * row-major rotation with row stride c2w_ld, e.g. 4 for camera_to_worlds[0]) -> GL axes -> cube lookup; no
 * direction tensor is materialised.  jitter: device [2,h,w] sub-pixel offsets (training, torch.rand_like) or
 * NULL for the +0.5 pixel centres (eval).  out [h*w, C]. */
int sgn_sky_fwd(int h, int w, float fx, float fy, float cx, float cy, const float *c2w, int c2w_ld,
                const float *jitter, int resolution, int channels, const float *tex, float *out,
                sgn_stream_t stream);
int sgn_sky_bwd(int h, int w, float fx, float fy, float cx, float cy, const float *c2w, int c2w_ld,
                const float *jitter, int resolution, int channels, const float *v_out, float *v_tex,
                sgn_stream_t stream);

/* Sky lookup fused with the reference's compositing (sgn_splatfacto.py:969-972):
 * out = min(rgb,1)*alpha + sky*(1-alpha); rgb/out [h*w,3], alpha [h*w], 3-channel texture.  sky_out (optional,
 * may be NULL) receives the raw sky colour (the reference's "sky" output).  The backward recomputes the lookup. */
int sgn_sky_blend_fwd(int h, int w, float fx, float fy, float cx, float cy, const float *c2w, int c2w_ld,
                      const float *jitter, int resolution, const float *tex, const float *rgb, const float *alpha,
                      float *out, float *sky_out, sgn_stream_t stream);
int sgn_sky_blend_bwd(int h, int w, float fx, float fy, float cx, float cy, const float *c2w, int c2w_ld,
                      const float *jitter, int resolution, const float *tex, const float *rgb, const float *alpha,
                      const float *v_out, float *v_rgb, float *v_alpha, float *v_tex, sgn_stream_t stream);

/* Fused photometric loss (sgn_splatfacto.py:1084-1087): Ll1 = mean |gt - pred| and
 * ssim = pytorch_msssim.SSIM(data_range, size_average=True, channel=3) of two [h,w,3] images (11-tap Gaussian window,
 * sigma 1.5, no padding, K = (0.01, 0.03)); h, w > 10.  out3 (device, 3 floats) receives Ll1, ssim and the reference's
 * weighted sum (1 - ssim_lambda) Ll1 + ssim_lambda (1 - ssim) (:1086-1087).  ws (>= sgn_l1_ssim_workspace_bytes) holds per-workgroup partial sums and, with
 * with_grad != 0, the SSIM partials sgn_l1_ssim_bwd needs (pass the same ws); the backward writes d loss / d pred
 * given gscale2 = (d loss/d Ll1, d loss/d ssim) as two DEVICE floats (no host sync between backward nodes). */
size_t sgn_l1_ssim_workspace_bytes(int h, int w, int with_grad);
int sgn_l1_ssim_fwd(int h, int w, const float *pred, const float *gt, float data_range,
                    float clamp_max /*pred is read as min(pred, clamp_max): the caller's rgb.clamp(max=1),
                                      sgn_splatfacto.py:969, folded in; pass INFINITY for none*/,
                    float ssim_lambda, float *out3, int with_grad, void *ws, size_t ws_bytes, sgn_stream_t stream);
int sgn_l1_ssim_bwd(int h, int w, const float *pred, const float *gt, float clamp_max, const void *ws,
                    const float *gscale2, float *v_pred, sgn_stream_t stream);

/* The same loss under the batch's pixel mask (sgn_splatfacto.py:1081-1087 in training, :1135-1151 in evaluation:
 * `gt_img *= mask; rgb *= mask` in front of the two terms), plus the mean squared error that PSNR needs.  mask: h*w
 * DEVICE bytes, non-zero = keep; NULL = no mask (the fourth output is still produced).  The kernels work on
 * min(pred, clamp_max) * m and gt * m; neither image is modified.  The reference's semantics, not the obvious ones:
 *   - both means keep their unmasked denominators, 3 h w for Ll1 (and the mse) and 3 (h-10) (w-10) for ssim: the
 *     reference multiplies and then calls .mean(); nothing is normalised by the number of kept pixels;
 *   - an SSIM window that straddles the mask edge sees zeros on both images; it is neither skipped nor reweighted;
 *   - the clamp is applied before the mask (:969 before :1083).
 * out4 (device, 4 floats) = Ll1, ssim, (1 - ssim_lambda) Ll1 + ssim_lambda (1 - ssim), mse = mean (gt m - pred m)^2.
 * ws >= sgn_l1_ssim_masked_workspace_bytes (its layout is NOT the unmasked entries': pass it to the masked backward
 * only).  The backward writes v_pred = m [pred <= clamp_max] (the unmasked expression on the masked images): an
 * exact 0 where m = 0.  Return codes: -1 h or w <= 10, -2 a NULL pred / gt / out4 / ws (backward: gscale2, v_pred),
 * -3 ws_bytes too small; all before anything is launched. */
size_t sgn_l1_ssim_masked_workspace_bytes(int h, int w, int with_grad);
int sgn_l1_ssim_masked_fwd(int h, int w, const float *pred, const float *gt, const unsigned char *mask,
                           float data_range, float clamp_max, float ssim_lambda, float *out4, int with_grad, void *ws,
                           size_t ws_bytes, sgn_stream_t stream);
int sgn_l1_ssim_masked_bwd(int h, int w, const float *pred, const float *gt, const unsigned char *mask,
                           float clamp_max, const void *ws, const float *gscale2, float *v_pred, sgn_stream_t stream);

/* The same loss with the ground truth as the data set caches it: gt is h*w*3 DEVICE bytes (uint8 [h,w,3], rows at
 * byte 3 w y, no alignment required), read by the kernels themselves; no float image is materialised.  A byte u stands
 * for the correctly rounded fp32 quotient u / 255, the value the reference caches (sgn_dataset.py:77,
 * astype("float32") / 255.0) and get_gt_img forms (sgn_splatfacto.py:1003-1012) -- NOT u * (1.0f / 255): 126 of the
 * 256 byte values differ in the last bit between the two.  The results are therefore bit for bit those of the masked
 * entries on that float image.  Everything else is sgn_l1_ssim_masked_fwd/bwd: mask may be NULL, the same out4, the same
 * ws (>= sgn_l1_ssim_masked_workspace_bytes, pass it to sgn_l1_ssim_gt8_bwd only) and the same return codes (-1 h or
 * w <= 10, -2 a NULL pred / gt / out4 / ws (backward: gscale2, v_pred), -3 ws_bytes too small), before any launch. */
int sgn_l1_ssim_gt8_fwd(int h, int w, const float *pred, const unsigned char *gt, const unsigned char *mask,
                        float data_range, float clamp_max, float ssim_lambda, float *out4, int with_grad, void *ws,
                        size_t ws_bytes, sgn_stream_t stream);
int sgn_l1_ssim_gt8_bwd(int h, int w, const float *pred, const unsigned char *gt, const unsigned char *mask,
                        float clamp_max, const void *ws, const float *gscale2, float *v_pred, sgn_stream_t stream);

/* One pyramid level of a batch's byte ground truth, for the reference's coarse-to-fine schedule (sgn_splatfacto.py:
 * 766-784, :822-823, :1055-1071: while d = 2 ** max(num_downscales - step // resolution_schedule, 0) > 1 the image is
 * resized with TF.resize(..., antialias=None) -- plain bilinear, align_corners=False -- and the mask and the semantic map
 * with InterpolationMode.NEAREST).  One launch reads image (uint8 [h,w,3]) and the optional mask / semantic (uint8 [h,w])
 * and writes image_out (float32 [oh,ow,3]) and mask_out / semantic_out (uint8 [oh,ow]); all DEVICE pointers, contiguous,
 * no alignment required, no workspace.  mask and mask_out are both NULL or both non-NULL, and so are semantic and
 * semantic_out.  The arithmetic contract, fp32 throughout, no FMA, per axis (in -> out):
 *   scale = (float)in / (float)out                        a true fp32 division
 *   src   = max(scale * ((float)dst + 0.5f) - 0.5f, 0.0f)
 *   i0    = min((int)src, in - 1);   i1 = i0 + (i0 < in - 1)
 *   l1    = src - (float)i0;         l0 = 1.0f - l1
 *   out   = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)    a, b on row i0h; a, c on column i0w
 *   a..d  = the correctly rounded (float)u / 255.0f of the four bytes, the quotient sgn_l1_ssim_gt8_fwd forms (NOT
 *           u * (1.0f / 255))
 *   mask, semantic: the source byte at min((int)floorf((float)dst * scale), in - 1) per axis, unchanged
 * Return codes, before any device work: -1 a dimension < 1 or > 16384, or oh > h, or ow > w; -2 a NULL image or
 * image_out, or a mask or semantic pair of which only one is given. */
int sgn_gt_downscale(int h, int w, int oh, int ow, const unsigned char *image, const unsigned char *mask,
                     const unsigned char *semantic, float *image_out, unsigned char *mask_out,
                     unsigned char *semantic_out, sgn_stream_t stream);

/* A frame's eval outputs as the bytes an image or video writer takes (the reference's scripts/render.py:159-273 runs every
 * output of every frame through colormaps.apply_colormap / apply_depth_colormap, moves the float32 result to the host
 * and leaves the float -> uint8 conversion to the writer; sgn_splatfacto.py:1134 builds the trainer's eval image the same
 * way).  One launch packs n_panels panels (1..SGN_FRAMES_MAX_PANELS), all h x w, into canvas, uint8
 * [canvas_h, canvas_w, 3]: panel i covers rows y0 .. y0 + h - 1 and columns x0 .. x0 + w - 1, so one call makes a column
 * of separate images or a side-by-side mosaic.  `panels` is a HOST array; it is copied into the kernel arguments (no
 * device buffer, no copy, no workspace, no host synchronisation).  src, lut and canvas are DEVICE pointers, contiguous,
 * no alignment required (16-byte aligned float sources, 4-byte aligned byte sources and canvas, with w, x0 and canvas_w
 * multiples of 4, take the 16-bytes-per-lane path; everything else goes byte by byte and returns the same bytes).
 * The rectangles must lie inside the canvas and must not overlap; bytes of the canvas outside them are not written.
 * THE ARITHMETIC IS A CONTRACT (tests/frames_oracle.py restates it), fp32, every operation rounded on its own:
 *   unit(v) = v > 0 ? (v < 1 ? v : 1) : 0                       clamp to [0, 1]; NaN -> 0, -inf -> 0, +inf -> 1
 *   q(x)    = (uint8) trunc(unit(x) * 255.0f + 0.5f)            the writers' float -> uint8 conversion (as recalled:
 *                                                               unpinned, no writer library was at hand)
 *   SGN_PANEL_RGB     src float32 [h,w,3]; each channel through q (apply_colormap returns 3-channel images unchanged)
 *   SGN_PANEL_SCALAR  src float32 [h,w];   t = (x - lo) / den   an IEEE fp32 division, not a reciprocal multiply
 *                                          t = clip(t, 0, 1), NaN propagating; then NaN -> 0      [together: unit(t)]
 *                                          t = 1 - t            if invert
 *                                          the pixel's three bytes are lut[(int) trunc(t * 255.0f)], lut uint8 [256,3]
 *                     lo = 0, den = 1 is apply_colormap's default path for accumulations (x * (1 - 0) + 0 is x); depth
 *                     takes lo = near and den = (float)((double)far - (double)near + 1e-10) (apply_depth_colormap)
 *   SGN_PANEL_BYTES   src uint8 [h,w,3], copied (the ground truth of a feed batch)
 * Return codes, before any device work: -1 h, w, canvas_h or canvas_w outside [1, 16384], n_panels outside
 * [1, SGN_FRAMES_MAX_PANELS], an unknown kind, a rectangle that leaves the canvas, two rectangles that overlap, a SCALAR
 * panel's den zero or not finite; -2 a NULL panels, canvas, src, or SCALAR panel's lut.  csrc/frame_pack.hip. */
#define SGN_FRAMES_MAX_PANELS 16
#define SGN_PANEL_RGB 0
#define SGN_PANEL_SCALAR 1
#define SGN_PANEL_BYTES 2
typedef struct sgn_panel {
    const void *src;    /* device: float32 [h,w,3] (RGB), float32 [h,w] (SCALAR), uint8 [h,w,3] (BYTES) */
    const uint8_t *lut; /* device: uint8 [256,3], SCALAR only (ignored otherwise) */
    int32_t kind;       /* SGN_PANEL_* */
    int32_t y0, x0;     /* top-left corner on the canvas */
    int32_t invert;     /* SCALAR: non-zero = t -> 1 - t */
    float lo, den;      /* SCALAR: t = (x - lo) / den */
} sgn_panel;
int sgn_frames_pack(int h, int w, int n_panels, const sgn_panel *panels /*host, [n_panels]*/, uint8_t *canvas,
                    int canvas_h, int canvas_w, sgn_stream_t stream);

/* Accumulation regularisers of the reference's loss dictionary, means over the n_pixels = H*W
 * entries of [H,W,1] accumulation images, one pass each way for both terms (either may be absent):
 *   out2[0] = mean([semantic == sky_value] * accumulation)      sgn_splatfacto.py:1090-1093 (losses["sky_accumulation"]
 *                                                               before its config multiplier; gt_semantic is int64)
 *   out2[1] = mean(-(o log o + (1 - o) log(1 - o))), o = clamp(object_acc, 1e-5, 1 - 1e-5)
 *                                                               sgn_splatfacto_scene_graph.py:386-389
 * accumulation == NULL skips the first term (out2[0] = 0), object_acc == NULL the second.  semantic holds n_pixels
 * integers of sem_bytes in {1, 4, 8} bytes (uint8 / bool mask with sky_value 1, int32, int64).  The backward takes
 * gscale2 = (d loss/d out2[0], d loss/d out2[1]) as two DEVICE floats and writes d loss/d accumulation and/or
 * d loss/d object_acc (NULL = not wanted); torch.clamp's rule: zero gradient outside [1e-5, 1 - 1e-5]. */
size_t sgn_acc_losses_workspace_bytes(int64_t n_pixels);
int sgn_acc_losses_fwd(int64_t n_pixels, const float *accumulation, const void *semantic, int sem_bytes,
                       int64_t sky_value, const float *object_acc, float *out2, void *ws, size_t ws_bytes,
                       sgn_stream_t stream);
int sgn_acc_losses_bwd(int64_t n_pixels, const void *semantic, int sem_bytes, int64_t sky_value,
                       const float *object_acc, const float *gscale2, float *v_accumulation, float *v_object_acc,
                       sgn_stream_t stream);

/* One torch.optim.Adam step (amsgrad = False, weight_decay = 0, maximize = False) over `count` tensors in a single
 * launch (optimiser set-up at sgn_config.py:71-108, eps = 1e-15).  Every array argument is a HOST
 * array of length `count`; params / grads / exp_avgs / exp_avg_sqs hold DEVICE pointers to contiguous fp32 tensors of
 * numel[i] elements; hyper-parameters are doubles (torch's Python scalars; rounded to fp32 once, where torch does);
 * steps[i] is the step count after the increment (>= 1). */
int sgn_adam_step(int count, float *const *params, const float *const *grads, float *const *exp_avgs,
                  float *const *exp_avg_sqs, const int64_t *numel, const double *lr, const double *beta1,
                  const double *beta2, const double *eps, const int64_t *steps, sgn_stream_t stream);

/* The same step for the rows a view saw (gsplat's SelectiveAdam, the 3DGS trainer's sparse Adam).  sgn_adam_step's
 * arguments plus three HOST arrays of length `count`: tensor i is rows[i] rows of numel[i] / rows[i] elements;
 * visible[i] is a DEVICE array of rows[i] entries (NULL allowed for SGN_ADAM_VIS_NONE only) of the type vis_kind[i]
 * names.  A visible row's param / exp_avg / exp_avg_sq get exactly what sgn_adam_step writes at steps[i], bit for bit;
 * an invisible row keeps its bits and is neither read nor written (a NaN or an infinity in its gradient or its moments
 * has no effect).  steps[i] is the caller's global count, as in SelectiveAdam: the bias corrections do not know how
 * often a row was seen, and the moments of an unseen row do not decay, so this is NOT torch.optim.Adam on a zero
 * gradient.  Empty tensors are skipped.  Every tensor's arguments are checked before the first launch; return codes:
 * -1 count < 0; -2 a NULL array; -3 numel[i] < 0 or steps[i] < 1; -4 a NULL tensor pointer with numel[i] > 0;
 * -5 vis_kind[i] outside 0..2; -6 rows[i] <= 0 with numel[i] > 0; -7 numel[i] % rows[i] != 0; -8 visible[i] NULL with
 * vis_kind[i] 1 or 2 and numel[i] > 0.  count == 0 returns 0.  Timed in the SGN_T_ADAM slot. */
#define SGN_ADAM_VIS_NONE 0 /* the tensor steps densely (the sky cube map, for instance) */
#define SGN_ADAM_VIS_U8 1   /* uint8 / bool, visible if nonzero */
#define SGN_ADAM_VIS_I32 2  /* int32, visible if > 0: the projection's radii as they are */
int sgn_adam_step_visible(int count, float *const *params, const float *const *grads, float *const *exp_avgs,
                          float *const *exp_avg_sqs, const int64_t *numel, const double *lr, const double *beta1,
                          const double *beta2, const double *eps, const int64_t *steps, const int64_t *rows,
                          const void *const *visible, const int32_t *vis_kind, sgn_stream_t stream);

/* Per-step densification statistics, SplatfactoModel.after_train (sgn_splatfacto.py:513-541), in one pass and without
 * the host syncs of boolean-mask indexing.  first != 0 initialises the three running buffers (the reference's
 * `is None` branches); max_dim = max(H, W) of the last rendered size. */
int sgn_densify_stats(int n, const float *xys_grad /*[n,2]*/, const int32_t *radii /*[n]*/, float max_dim, int first,
                      float *xys_grad_norm /*[n]*/, float *vis_counts /*[n]*/, float *max_2dsize /*[n]*/,
                      sgn_stream_t stream);

/* THE REFINEMENT ITSELF: SplatfactoModel.refinement_after / split_gaussians / dup_gaussians / cull_gaussians and the
 * optimiser-state surgery dup_in_optim / remove_from_optim (sgn_splatfacto.py:459-720) in three steps over one
 * caller-allocated workspace, ws >= sgn_densify_workspace_bytes(n) (depends on n only; 0 for n <= 0), which carries the
 * per-row flags and per-block offsets from one step to the next.  Decisions, output order and values are those of
 * sgn_rast.densify.Densifier's torch engine: kept originals in input order, then the children of the kept split parents
 * sample-major (like .repeat(samps, 1)), then the kept duplicates in input order.  Integer sums in a fixed order, no
 * atomics: bit-identical results for the same input.  All asynchronous on `stream`; n == 0 returns 0 without a launch.
 * Return codes: -1 n / n_out out of range (n * (n_split_samples + 2) must fit an int32), -2 n_split_samples outside
 * [1, 64], -3 a required pointer is NULL (or an output aliases its input), -4 image_dim <= 0 with densify on,
 * -5 workspace too small, -6 bad tensor table, -7 quats not 16-byte aligned.  csrc/densify.hip.
 *
 * sgn_densify_decide: one lane per INPUT Gaussian.  With densify != 0 (:571-612)
 *     high = (xys_grad_norm / vis_counts) * 0.5 * image_dim > densify_grad_thresh        (x/0 = inf is high, 0/0 is not)
 *     split = (max exp(log_scales) > densify_size_thresh  [| max_2dsize > split_screen_size]) & high
 *     dup = (max exp(log_scales') <= densify_size_thresh) & high,  log_scales' = log(exp(log_scales) / 1.6) for a split
 *           parent (the reference shrinks in place before it looks for duplicates: a Gaussian can be both)
 * and the cull test of :648-672 as the reference applies it to [old, children, dups]: every split parent goes;
 * sigmoid(opacity_logits) < cull_alpha_thresh, and with too_big_culls != 0 max exp(log_scales') > cull_scale_thresh
 * [| max_2dsize > cull_screen_size, new rows carrying max_2dsize = 0], remove a row.  The bracketed screen-size tests
 * run with screen_size_tests != 0 (step < stop_screen_size_at); densify == 0 is the cull-only refinement after
 * stop_split_at (xys_grad_norm / vis_counts may be NULL then; max_2dsize may be NULL without the screen-size tests).
 *
 * sgn_densify_scan: the exclusive offsets of every block of rows, and totals8 (DEVICE int32[8], read back once by the
 * host): [0] kept originals, [1] split parents (n_splits: the noise has n_split_samples * n_splits rows), [2] split
 * parents whose children survive, [3] surviving duplicates — N' = [0] + n_split_samples * [2] + [3] — then the
 * reference's counters with its multiplicity: [4] high_grads_count, [5] refine_dups_count, [6]
 * refine_culls_toobigs_count (split parents and new rows included), [7] 0; refine_splits_count = [1].
 *
 * sgn_densify_apply: two launches.  The first writes src[n_out] (the input row output row r derives from) and
 * kind[n_out] (0 a bit-exact copy, -1 a duplicate, 1 + noise row of child k = 1 + k * n_splits + rank of the parent among
 * all split parents).  The second writes `count` (<= 24) output tensors of n_out rows from their n-row inputs; HOST
 * arrays of length count: DEVICE pointers inputs[i] / outputs[i] (contiguous fp32, never aliased), row_floats[i] floats
 * per row and roles[i]: 0 a parameter whose new rows copy their source row; 1 `means` (a child's row is
 * R(q / |q|) (exp(log_scales) * noise[row]) + mean, R by gsplat's quat_to_rotmat); 2 `log_scales` (children and the
 * duplicate of a split parent get log(exp(.) / 1.6)); 3 an Adam moment (new rows are zeros).  means / log_scales /
 * quats are the INPUT parameters [n,3] / [n,3] / [n,4], noise [noise_rows,3] the caller's normal deviates.  Elements
 * are indexed in 64 bits.  n_out == 0 returns 0 without a launch. */
size_t sgn_densify_workspace_bytes(int n);
int sgn_densify_decide(int n, const float *xys_grad_norm /*[n]*/, const float *vis_counts /*[n]*/,
                       const float *max_2dsize /*[n]*/, const float *log_scales /*[n,3]*/,
                       const float *opacity_logits /*[n]*/, float densify_grad_thresh, float densify_size_thresh,
                       float split_screen_size, float cull_alpha_thresh, float cull_scale_thresh,
                       float cull_screen_size, float image_dim, int n_split_samples, int densify,
                       int screen_size_tests, int too_big_culls, void *ws, size_t ws_bytes, sgn_stream_t stream);
int sgn_densify_scan(int n, void *ws, size_t ws_bytes, int32_t *totals8 /*device int32[8]*/, sgn_stream_t stream);
int sgn_densify_apply(int n, int n_out, int n_split_samples, int64_t noise_rows, const float *means,
                      const float *log_scales, const float *quats, const float *noise /*[noise_rows,3]*/, int count,
                      const float *const *inputs, float *const *outputs, const int32_t *row_floats,
                      const int32_t *roles, int32_t *src /*[n_out]*/, int32_t *kind /*[n_out]*/, const void *ws,
                      size_t ws_bytes, sgn_stream_t stream);

/* FIXED-BUDGET MCMC REFINEMENT ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's MCMCStrategy; no
 * counterpart in the reference; decided here from the published algorithm, unpinned): dead Gaussians teleported onto
 * live ones sampled by opacity, growth up to a cap, opacity-gated noise on the means.  The arithmetic contract is the
 * header comment of csrc/mcmc.hip; sgn_rast.mcmc.MCMCDensifier's torch engine restates it and takes the same integer
 * decisions bit for bit.  One phase (relocate, or grow) is weights -> scan -> [host reads totals2] -> draw ->
 * relocation -> apply over one caller-allocated workspace, ws >= sgn_mcmc_workspace_bytes(n) (0 for n <= 0), which
 * carries the block sums, the totals, the per-row draw counts and the per-row owning draw between the steps.  All
 * asynchronous on `stream`; n == 0 (and k == 0 where there is a k) returns 0 without a launch.  Return codes: -1 n / k
 * out of range (n + k must fit an int32; relocate: k <= n), -2 n_max outside [1, 51], -3 a required pointer is NULL (or
 * relocate's outputs[i] != inputs[i], grow's outputs[i] == inputs[i]), -4 mode not 0 / 1, -5 workspace too small,
 * -6 bad tensor table, -7 quats not 16-byte aligned.
 *
 * sgn_mcmc_weights: one lane per row.  o = 1 / (1 + exp(-(double)logit)); dead[i] = o <= (double)min_opacity;
 *     w[i] = floor(o * 2^24 + 0.5), and 0 for a dead row when relocate != 0.
 * sgn_mcmc_scan: prefix[i] = the exclusive int64 sum of w (a block scan, then a scan of the block sums);
 *     dead_rows[j] = the j-th dead row in row order; totals2 (DEVICE int64[2], read back once per phase) = [n_dead, total].
 * sgn_mcmc_draw: one lane per draw j < k: h = mix64(mix64(j + 1) ^ key), t = (h >>> 1) mod total, src[j] = the row with
 *     prefix[s] <= t < prefix[s] + w[s] (binary search); then ratio[j] = min(n_max, 1 + number of draws that chose
 *     src[j]).  total == 0 is the caller's case to skip.
 * sgn_mcmc_relocation: staging[j] = {logit', log_scales'[3]} of draw j, in fp64 from row src[j]'s CURRENT logit and
 *     log-scales (nothing has been written yet), rounded to fp32 once.
 * sgn_mcmc_apply: `count` (<= 24) tensors by HOST arrays of DEVICE pointers inputs[i] / outputs[i] (contiguous fp32),
 *     row_floats[i] and roles[i]: 0 a parameter whose target rows copy their source row, 1 the opacity logits
 *     (row_floats 1), 2 the log-scales (row_floats 3), 3 an Adam moment.  mode 0, relocate, IN PLACE (outputs[i] ==
 *     inputs[i], n rows): row targets[j] becomes row src[j] with the staged values, row src[j] gets the staged values
 *     and zeroed moments; targets' moments and every other row keep their bits.  mode 1, grow (outputs of n + k rows,
 *     never aliased; targets ignored): rows < n copy, sources with the staged values and their moments unchanged; row
 *     n + j copies src[j] with the staged values and zero moments.
 * sgn_mcmc_noise: the per-step pass, one lane per row: three hashed normal deviates (fp64 Box-Muller on the row's own
 *     counter hash, rounded to fp32; z_out [n,3] nullable receives them), then in fp32
 *     means += R diag(exp(log_scales))^2 R^T ((z * g) * scaler), g = 1 / (1 + exp(-100 ((1 - sigmoid(logit)) - 0.995))). */
size_t sgn_mcmc_workspace_bytes(int n);
int sgn_mcmc_weights(int n, const float *opacity_logits /*[n]*/, float min_opacity, int relocate, int32_t *w /*[n]*/,
                     uint8_t *dead /*[n]*/, void *ws, size_t ws_bytes, sgn_stream_t stream);
int sgn_mcmc_scan(int n, const int32_t *w, const uint8_t *dead, int64_t *prefix /*[n]*/, int32_t *dead_rows /*[n]*/,
                  void *ws, size_t ws_bytes, int64_t *totals2 /*device int64[2]*/, sgn_stream_t stream);
int sgn_mcmc_draw(int n, int k, int64_t key, int n_max, const int64_t *prefix, int32_t *src /*[k]*/,
                  int32_t *ratio /*[k]*/, void *ws, size_t ws_bytes, sgn_stream_t stream);
int sgn_mcmc_relocation(int n, int k, const float *opacity_logits, const float *log_scales /*[n,3]*/, float min_opacity,
                        const int32_t *src, const int32_t *ratio, float *staging /*[k,4]*/, sgn_stream_t stream);
int sgn_mcmc_apply(int mode, int n, int k, const int32_t *src, const int32_t *targets, const float *staging, int count,
                   const float *const *inputs, float *const *outputs, const int32_t *row_floats, const int32_t *roles,
                   const void *ws, size_t ws_bytes, sgn_stream_t stream);
int sgn_mcmc_noise(int n, int64_t key, float scaler, float *means /*[n,3]*/, const float *log_scales /*[n,3]*/,
                   const float *quats /*[n,4]*/, const float *opacity_logits /*[n]*/, float *z_out /*[n,3] or NULL*/,
                   sgn_stream_t stream);

/* Exact k-nearest neighbours of 3-D points (SplatfactoModel.populate_modules, sgn_splatfacto.py:260-264: the reference's
 * k_nearest_sklearn, :439-457, sklearn NearestNeighbors(k + 1) with the first column dropped).  For every row i of
 * points [n,3] (finite fp32; non-finite input gives unspecified rows, never an out-of-bounds access): dist[i, :] = the k
 * smallest |x_i - x_j| over j != i, ascending, as fp32 direct differences; idx[i, :] = those j (distinct, never i; on
 * equal distances the choice among them is this library's, not sklearn's).  1 <= k <= 16, n > k (else rc < 0).
 * Deterministic: bit-identical results for the same input.  visited (nullable, device int64): ADDS the number of
 * candidate distances evaluated (the work bound the tests check).  Asynchronous on `stream`, no host synchronisation;
 * ws >= sgn_knn_workspace_bytes(n, k), which depends on n and k only (0 when n is out of range).  csrc/knn.hip. */
size_t sgn_knn_workspace_bytes(int n, int k);
int sgn_knn(int n, int k, const float *points /*[n,3]*/, float *dist /*[n,k]*/, int32_t *idx /*[n,k]*/,
            int64_t *visited /*nullable: device int64, += candidate distances evaluated*/, void *ws, size_t ws_bytes,
            sgn_stream_t stream);

/* NEAREST NEIGHBOUR ACROSS TWO CLOUDS (the primitive of the reference's LiDAR chamfer metric,
 * street_gaussians_ns/data/utils/geometric_metric.py:59-69: open3d's compute_point_cloud_distance, the exact distance to
 * the nearest point of the other cloud).  For every row q of query [n_query,3]: dist[q] = the smallest |query_q - target_j|
 * over ALL rows j of target [n_target,3] as an fp32 direct difference, idx[q] = that j (idx nullable; no row is excluded:
 * the clouds are unrelated; on equal distances the choice among them is this library's).  Finite fp32 input; non-finite
 * input gives unspecified rows, never an out-of-bounds access.  1 <= n_target, n_query <= 2^30 (else rc < 0).  The tree of
 * sgn_knn is built over the target, the queries are sorted along the target's Morton curve and 64 neighbouring queries
 * walk the tree together (n_query * 16 <= n_target: one wave per query instead, no query sort).  Deterministic:
 * bit-identical results for the same input.  visited (nullable, device int64): ADDS the number of candidate distances
 * evaluated.  Asynchronous on `stream`, no host synchronisation;
 * ws >= sgn_cloud_nn_workspace_bytes(n_target, n_query), which depends on the two counts only (0 when one is out of
 * range).  csrc/cloud_nn.hip. */
size_t sgn_cloud_nn_workspace_bytes(int n_target, int n_query);
int sgn_cloud_nn(int n_target, const float *target /*[n_target,3]*/, int n_query, const float *query /*[n_query,3]*/,
                 float *dist /*[n_query]*/, int32_t *idx /*[n_query], may be NULL*/, int64_t *visited /*may be NULL*/,
                 void *ws, size_t ws_bytes, sgn_stream_t stream);

/* LiDAR SEEDING (the reference's scripts/pythons/pcd2colmap_points3D.py:114-235 and extract_object_pts.py:114-273: LiDAR
 * points coloured from the camera image they project into, sorted into the background cloud and one cloud per tracked
 * box).  One call pair handles one sweep against one camera and at most SGN_SEED_MAX_BOXES boxes.  HOST arguments:
 * l2w12 (LiDAR -> world, 3x4 row-major), min_z, `boxes` (n_boxes rows; the caller has applied the reference's 1.1
 * scale to `half`) and `cam`; they are copied into kernel arguments.  DEVICE: points [n,3] fp32 in the LiDAR frame (rows
 * may hold NaN), image [height,width,3] uint8.
 * THE ARITHMETIC IS A CONTRACT, fp32 throughout, no contraction, IEEE division; a float32 restatement reproduces every
 * output bit for bit (tests/seed_oracle.py):
 *     pw[r]   = ((L[r][0] x + L[r][1] y) + L[r][2] z) + L[r][3]                      L = l2w12
 *     live    = no NaN in the row  &  z > min_z (strict)  &  !(|pw.x| > 1e5)
 *     loc[k]  = (R[0][k] d[0] + R[1][k] d[1]) + R[2][k] d[2],  d = pw - center        R = rot (box -> world)
 *     inside  = |loc[k]| <= half[k] for k = 0, 1, 2                                   (closed: a face is inside)
 *     pc      = w2c applied to pw, parenthesised as pw
 *     fu      = (fx pc.x + cx pc.z) / pc.z,  fv = (fy pc.y + cy pc.z) / pc.z
 *     visible = pc.z > 0  &  fu, fv finite  &  0 <= trunc(fu) < width  &  0 <= trunc(fv) < height
 *               (truncation toward zero, decided in floating point: fu in (-1, 0) is column 0, as numpy's astype(int))
 * sgn_seed_classify writes the per-point verdicts and per-block counts into ws and totals (DEVICE int32[n_boxes + 2], read
 * back once by the host to size the outputs): [b] rows of box b (live & inside_b & visible), [n_boxes] background rows
 * (live & visible & inside no box), [n_boxes + 1] live points.  sgn_seed_emit, on the same ws / points / image size,
 * writes the rows, every segment in input point order: the object rows of box 0, then box 1, ... (a point inside two boxes
 * has a row in both) as obj_local [obj_rows,3] = loc, obj_rgb [obj_rows,3] = the image's 3 bytes at (trunc(fv),
 * trunc(fu)), obj_src [obj_rows] = the point's index; the background rows as bg_world = pw, bg_rgb, bg_src.  obj_rows /
 * bg_rows are the capacities of the arrays (rows past them are not written; 0 with NULL arrays skips that kind).
 * Integer sums in a fixed order, no atomics: stable and bit-identical from run to run.  Asynchronous on `stream`.
 * ws >= sgn_seed_workspace_bytes(n, n_boxes) (0 when an argument is out of range).  Return codes: -1 n outside
 * [1, SGN_SEED_MAX_POINTS]; -2 n_boxes outside [0, SGN_SEED_MAX_BOXES]; -3 width / height outside
 * [1, SGN_SEED_MAX_IMAGE_DIM]; -4 a required pointer is NULL; -5 workspace too small; -6 obj_rows / bg_rows out of range.
 * csrc/seed.hip. */
#define SGN_SEED_MAX_BOXES 64
#define SGN_SEED_MAX_POINTS (1 << 27)
#define SGN_SEED_MAX_IMAGE_DIM 16384
typedef struct sgn_seed_box {
    float center[3]; /* world */
    float rot[9];    /* box -> world, 3x3 row-major */
    float half[3];   /* half extents along the box axes */
} sgn_seed_box;
typedef struct sgn_seed_cam {
    float w2c[12];   /* world -> camera, 3x4 row-major */
    float fx, fy, cx, cy;
    int32_t width, height;
} sgn_seed_cam;
size_t sgn_seed_workspace_bytes(int n, int n_boxes);
int sgn_seed_classify(int n, const float *points /*[n,3]*/, const float *l2w12 /*host*/, float min_z, int n_boxes,
                      const sgn_seed_box *boxes /*host, [n_boxes]*/, const sgn_seed_cam *cam /*host*/, void *ws,
                      size_t ws_bytes, int32_t *totals /*device int32[n_boxes + 2]*/, sgn_stream_t stream);
int sgn_seed_emit(int n, const float *points /*[n,3]*/, int n_boxes, const uint8_t *image /*[height,width,3]*/,
                  int width, int height, const void *ws, size_t ws_bytes, float *obj_local, uint8_t *obj_rgb,
                  int32_t *obj_src, int64_t obj_rows, float *bg_world, uint8_t *bg_rgb, int32_t *bg_src, int64_t bg_rows,
                  sgn_stream_t stream);

/* LiDAR DEPTH (the reference supervises depth against images made offline, point by point on the CPU:
 * data_utils.get_depth_image_from_path loads them).  Sweeps become a per-pixel target on the device, and the pair
 * features.expected_depth renders — dsum = sum_g depth_g alpha_g T_g and alpha, both [H,W] — becomes a loss with its
 * gradient and the evaluation depth metrics.  DEVICE: points, depth, out, dsum, alpha, target, mask, loss_out,
 * count_out / count, v_loss, v_dsum, v_alpha, out5, ws.  HOST: l2w12, cam, the scalars.  Asynchronous on `stream`, no host
 * read anywhere.  fp32 throughout, no contraction, IEEE division; tests/lidar_depth_oracle.py restates all of it.
 * TARGET, three calls, so that several sweeps and several LiDARs land in one camera's image:
 *   sgn_lidar_depth_begin   depth [height,width] = +inf (the bit pattern 0x7f800000).
 *   sgn_lidar_depth_splat   one sweep: points [n,3] in the LiDAR frame (rows may hold NaN).  pw, live, pc, fu, fv and
 *       visible are those of "LiDAR SEEDING" above, same parenthesisation, same truncation rule.  A point COUNTS when
 *       it is live, visible and pc.z <= max_depth; each counted point does one atomic minimum on the uint32 view of
 *       depth[trunc(fv)][trunc(fu)] with the bits of pc.z (positive floats order as unsigned integers).  The nearest
 *       return wins whatever the arrival order: bit-identical from run to run, and two sweeps splatted in turn equal
 *       their concatenation splatted once.
 *   sgn_lidar_depth_finish  out [height,width], which must not alias depth: 0 where a pixel has no return; a pixel with
 *       return z keeps it iff  z * (1 - rel_tol) <= m,  m the minimum return over the (2 radius + 1)^2 window clipped
 *       to the image, the pixel itself included — else 0.  The product is ONE fp32 multiply of z by the fp32 constant
 *       1.0f - rel_tol, formed on the host.  This is the occlusion filter the LiDAR / camera parallax makes necessary:
 *       the LiDAR sits above the camera and sees background between foreground returns.  radius 0 keeps every return.
 * LOSS, one thread per pixel; mask: bytes [H,W], non-zero = keep, NULL = no mask (sgn_rast.loss.check_mask's convention).
 * With D = dsum / alpha and z = target:
 *     counted = z > 0  &  alpha > 1e-3  &  dsum > 0  &  (mask == NULL | mask != 0)
 *     kind 0 (l1):      l = |D - z|            kind 1 (inverse):  l = |1 / D - 1 / z|
 *     loss = (sum over counted of l) / max(count, 1)
 * (alpha > 1e-3 is the reference's validity rule for its depth output, sgn_splatfacto.py:995.)  The fp32 per-pixel terms
 * go into an fp64 sum: per wave with shuffles, across the block's waves through LDS, one fp64 and one integer atomic per
 * block; a one-thread launch writes loss_out[0] and count_out[0] (int32).  sgn_depth_loss_bwd reads count and v_loss from
 * device memory; with g = v_loss / max(count, 1), s = sign(D - z) resp. sign(1 / D - 1 / z), 0 at equality:
 *     l1:       v_dsum = (g s) / alpha                   v_alpha = -v_dsum D
 *     inverse:  v_dsum = (-(g s) / (D D)) / alpha        v_alpha = -v_dsum D
 * Uncounted pixels get exact zeros in both; count == 0 gives loss 0 and all-zero gradients, no NaN.
 * METRICS: sgn_depth_metrics, the same inputs and the same `counted`, one launch; out5 = abs_rel (mean |D - z| / z),
 * rmse (sqrt(mean (D - z)^2)), mae (mean |D - z|), delta1 (the share with max(D / z, z / D) < 1.25), count (as fp32:
 * exact up to 2^24 counted pixels); all 0 without a counted pixel.
 * ws: SGN_DEPTH_LOSS_WS_BYTES of device memory, cleared by the call.  Return codes: -1 n outside
 * [1, SGN_SEED_MAX_POINTS]; -2 max_depth <= 0, radius outside [0, SGN_LIDAR_DEPTH_MAX_RADIUS], rel_tol outside [0, 1) or
 * kind outside {0, 1}; -3 width / height outside [1, SGN_SEED_MAX_IMAGE_DIM]; -4 a required pointer is NULL; -5 workspace
 * too small; -6 out aliases depth.  csrc/lidar_depth.hip. */
#define SGN_LIDAR_DEPTH_MAX_RADIUS 8
#define SGN_DEPTH_LOSS_WS_BYTES 64
#define SGN_DEPTH_LOSS_L1 0
#define SGN_DEPTH_LOSS_INVERSE 1
int sgn_lidar_depth_begin(float *depth /*[height,width]*/, int height, int width, sgn_stream_t stream);
int sgn_lidar_depth_splat(int n, const float *points /*[n,3]*/, const float *l2w12 /*host*/, float min_z, float max_depth,
                          const sgn_seed_cam *cam /*host*/, float *depth /*[height,width]*/, sgn_stream_t stream);
int sgn_lidar_depth_finish(const float *depth /*[height,width]*/, int height, int width, int radius, float rel_tol,
                           float *out /*[height,width]*/, sgn_stream_t stream);
int sgn_depth_loss_fwd(int img_h, int img_w, const float *dsum, const float *alpha, const float *target,
                       const unsigned char *mask /*may be NULL*/, int kind, float *loss_out, int32_t *count_out, void *ws,
                       size_t ws_bytes, sgn_stream_t stream);
int sgn_depth_loss_bwd(int img_h, int img_w, const float *dsum, const float *alpha, const float *target,
                       const unsigned char *mask /*may be NULL*/, int kind, const float *v_loss, const int32_t *count,
                       float *v_dsum, float *v_alpha, sgn_stream_t stream);
int sgn_depth_metrics(int img_h, int img_w, const float *dsum, const float *alpha, const float *target,
                      const unsigned char *mask /*may be NULL*/, float *out5, void *ws, size_t ws_bytes,
                      sgn_stream_t stream);

/* ANTIALIASED OPACITY (rasterize_mode "antialiased", sgn_splatfacto.py:214-222, :947: the multiply the reference leaves
 * commented out).  The effective opacity of row i from its logit l and the projection's compensation factor c
 * (sqrt(max(0, det / det_blurred)); 0 on a culled row), fp32, no contraction:
 *   s   = 1.f / (1.f + expf(-l))              the sigmoid as the rasterizer's row build spells it
 *   o   = s * c
 *   v_l = ((v_o * c) * s) * (1.f - s)         left to right, as the rasterizer's gradient unpack chains its sigmoid
 *   v_c = v_o * s
 * so a culled row has o = 0 and v_l = 0, and with c == 1.0f o has exactly the bits the fused rasterizer forms from the
 * logit itself.  `opacities` is handed on as PROBABILITIES (opacity_is_logit = 0) to every raster / binning entry; v_o is
 * the sum of those passes' opacity gradients, v_c goes to the projection backward as v_compensation.
 * One row per lane, 4-byte accesses: the arrays need no more than float alignment.  v_opacity_logits / v_compensation:
 * either may be NULL (not wanted); both NULL returns 0 without a launch, as n == 0 does.
 * Return codes: -1 n < 0; -2 a required pointer is NULL. */
int sgn_aa_opacity_fwd(int n, const float *opacity_logits, const float *compensation, float *opacities,
                       sgn_stream_t stream);
int sgn_aa_opacity_bwd(int n, const float *opacity_logits, const float *compensation, const float *v_opacities,
                       float *v_opacity_logits, float *v_compensation, sgn_stream_t stream);

/* ROLLING SHUTTER (no upstream counterpart: the reference renders a global shutter).  The sensor reads line c of the
 * shutter axis s (SGN_SHUTTER_ROWS: s = y, extent E = img_h; SGN_SHUTTER_COLS: s = x, E = img_w; o is the other axis)
 * at time tau(c) = T * (c / E - 0.5) around the mid-exposure pose the projection ran at; pixel centres sit at r + 0.5,
 * T < 0 reverses the readout.  `lin` = R (v_cam - v_obj) and `ang` = R w_cam are the camera's velocity relative to the
 * row's object and its angular velocity, rotated into the CAMERA frame by the host (R = viewmat[:3,:3]); with
 * object_ids / lin_table [n_objects, 3] the row's `lin` is lin_table[object_ids[i]] (an id outside the table reads its
 * nearest row), else the struct's.  Per row with radii > 0, from the projection's (u, z, r, Q = [[q0, q1], [q1, q2]]),
 * fp32, no contraction, every expression evaluated as written (left to right):
 *   u    = u - margin                                  (both axes; the projection ran on a padded image, see below)
 *   x    = (u_x - cx) * (z + 1e-6f) / fx               y = (u_y - cy) * (z + 1e-6f) / fy        p = (x, y, z)
 *   pd   = -l - w x p:   pd_x = -l_x - (w_y * z - w_z * y),  pd_y = -l_y - (w_z * x - w_x * z),  pd_z = -l_z - (w_x * y - w_y * x)
 *   a_x  = fx * (pd_x - (x / z) * pd_z) / z            a_y = fy * (pd_y - (y / z) * pd_z) / z    (screen velocity)
 *   g    = a * T / E          k = 1.f - g_s            b = -g_o                A = I - g e_s^T
 *   u'_s = (u_s - 0.5f * T * a_s) / k                  tau' = T * (u'_s / E - 0.5f)
 *   u'_o = u_o + a_o * tau'                            depth' = z + pd_z * tau'
 *   Q'   = A^T Q A:   Q'_oo = Q_oo,   Q'_os = Q_oo * b + q1 * k,   Q'_ss = b * Q'_os + k * (q1 * b + Q_ss * k)
 *   c    = g_o / k,  d = 1.f + g_s / k,  t = 1.f + c * c + d * d                (A^-1 = I + g e_s^T / k)
 *   sigma = sqrtf(0.5f * (t + sqrtf(fmaxf(0.f, t * t - 4.f * (d * d)))))        (its largest singular value)
 *   r'   = (int)ceilf((float)r * sigma)                conservative: never below the sheared footprint's 3-sigma radius
 *   num_tiles_hit' = the area of sgn tile bbox(u', r') on the REAL image's tile grid under `semantics`, as the projection
 * A row is culled when k < 0.5f (the point nearly keeps pace with the shutter), depth' <= clip_thresh or the tile area
 * is 0: xys', depths', radii', num_tiles_hit' are 0 as the projection writes them, conics' holds Q' (the projection
 * writes its conic before the area test, too).  A row with radii <= 0 comes out culled with its conic unchanged.
 * With l = w = 0 every product above is with an exact 0 or 1: k = 1, b = c = 0, sigma = 1, and — margin = 0 — all five
 * outputs equal the inputs bit for bit; that only holds without contraction or reassociation (-ffp-contract=off).
 * The compensation factor is not touched (and not an argument).
 * `margin` m >= 0 (pixels): the caller ran the projection on a virtual image (img_h + 2 m, img_w + 2 m) with the
 * principal point at (cx + m, cy + m), so that a Gaussian just off the image at mid-exposure survives to be moved onto
 * the border lines; the struct carries the REAL img_h, img_w, cx, cy.  Side effects of m > 0: the projection's
 * 1.3 * tan(fov / 2) Jacobian clamp is taken from the padded size, and u carries the rounding of adding and
 * subtracting m (at most one ulp of img_w + 2 m on an unmoved row).
 * sgn_rolling_shutter_bwd: the analytic vjp of the above with respect to (u, z, Q), including the dependence of a on u
 * and z; the velocities are data.  radii_out is the forward's: a row culled there gets zero gradients.  v_depths_out
 * may be NULL (no gradient arrives through the depths).
 * One row per lane, 4-byte accesses: the arrays need no more than float alignment.  n == 0 returns 0 without a launch.
 * Return codes: -1 n < 0; -2 rs or a required pointer is NULL; -3 axis is neither constant; -4 bad image size / block
 * width (2..16); -5 fx or fy <= 0, margin < 0; -6 exactly one of object_ids / lin_table given, or n_objects < 1 with
 * them.  csrc/rolling_shutter.hip. */
#define SGN_SHUTTER_ROWS 0
#define SGN_SHUTTER_COLS 1
typedef struct sgn_shutter {
    float fx, fy, cx, cy;    /* the real camera's intrinsics */
    float lin[3];            /* R (v_cam - v_obj), used when lin_table is NULL */
    float ang[3];            /* R w_cam */
    float duration;          /* T, seconds, signed */
    float margin;            /* m, pixels */
    float clip_thresh;       /* the projection's */
    int32_t axis;            /* SGN_SHUTTER_ROWS | SGN_SHUTTER_COLS */
    int32_t img_h, img_w, block_width;
    int32_t semantics;       /* SGN_SEM_* bits (the tile bbox's) */
} sgn_shutter;
int sgn_rolling_shutter_fwd(int n, const float *xys, const float *depths, const int32_t *radii, const float *conics,
                            const int32_t *object_ids /*[n] or NULL*/, const float *lin_table /*[n_objects,3] or NULL*/,
                            int n_objects, const sgn_shutter *rs, float *xys_out, float *depths_out,
                            int32_t *radii_out, float *conics_out, int32_t *num_tiles_hit_out, sgn_stream_t stream);
int sgn_rolling_shutter_bwd(int n, const float *xys, const float *depths, const float *conics,
                            const int32_t *radii_out, const int32_t *object_ids /*[n] or NULL*/,
                            const float *lin_table /*[n_objects,3] or NULL*/, int n_objects, const sgn_shutter *rs,
                            const float *v_xys_out, const float *v_depths_out /*may be NULL*/,
                            const float *v_conics_out, float *v_xys, float *v_depths, float *v_conics,
                            sgn_stream_t stream);

/* BILATERAL GRID (per-image colour correction: cameras of a street rig meter on their own; gsplat's trainer answers
 * with a bilateral grid per image, the original Street Gaussians code with a 3x4 affine per image / sensor, which is the
 * 1 x 1 x 1 grid).  grid: g[L, Hg, Wg, 12] float32, cell-major, coefficient 4 r + c = row r, column c of a 3x4 affine
 * (c = 3: the bias), 16-byte aligned.  rgb / out / v_out / v_rgb: the first n_pix pixels, row-major, of an H x W image,
 * 3 floats each (0 <= n_pix <= H * W; the whole image is n_pix = H * W).  For pixel (i, j) with colour p = (R, G, B):
 *     gx = (j + 0.5) / W * (Wg - 1)          gy = (i + 0.5) / H * (Hg - 1)          (IEEE division)
 *     luma = 0.299 R + 0.587 G + 0.114 B     gz = clamp(luma, 0, 1) * (L - 1)
 *     x0 = floor(gx), x1 = min(x0 + 1, Wg - 1), fx = gx - x0                        and the same for y and z
 *     A = the trilinear mix of the eight cells as NESTED LERPS a + f * (b - a): z innermost, then x, then y
 *     out_r = A[r,0] R + A[r,1] G + A[r,2] B + A[r,3]                               (left to right)
 * i.e. grid_sample(align_corners=True, padding_mode="border") on (x, y, luma) in [0,1]^3 and the affine.  The lerp form
 * is part of the contract: a grid whose cells are all the identity affine returns rgb bit for bit.  fp32, no contraction.
 * sgn_bilagrid_slice_bwd, with w_cell the product of a cell's three lerp weights, dA = A|z1 - A|z0 (the innermost lerps'
 * differences mixed over x and y as A is; zero when z0 == z1) and lw the three luma weights:
 *     v_grid[cell][4 r + c] += w_cell * v_out_r * (R, G, B, 1)[c]
 *     v_rgb_k = sum_r v_out_r A[r,k] + lw_k * (L - 1) * [0 < luma < 1] * sum_r v_out_r * (dA[r,:] . (R, G, B, 1))
 * v_grid [L, Hg, Wg, 12] is ADDED INTO (the caller clears it) with float atomics after an on-chip sum: its last bits
 * depend on arrival order; out and v_rgb are plain stores, bit-identical from run to run.  v_rgb / v_grid: either may be
 * NULL (not wanted); both NULL returns 0 without a launch, as n_pix == 0 does.  No workspace.
 * Return codes: -1 L, Hg, Wg, H or W < 1, H or W > 16384, more than 2^27 cells, n_pix outside [0, H * W]; -2 a required
 * pointer is NULL; -3 grid is not 16-byte aligned.  csrc/bilagrid.hip. */
int sgn_bilagrid_slice_fwd(int L, int Hg, int Wg, const float *grid, int H, int W, int n_pix, const float *rgb,
                           float *out, sgn_stream_t stream);
int sgn_bilagrid_slice_bwd(int L, int Hg, int Wg, const float *grid, int H, int W, int n_pix, const float *rgb,
                           const float *v_out, float *v_rgb, float *v_grid, sgn_stream_t stream);

/* BATCHED VIEWS (no upstream counterpart; gsplat 1.x takes [C] cameras per call).  B = n_views cameras share one image
 * size (img_h, img_w), 16x16 tiles and one set of N Gaussians in the fused front end's raw form (means, log-scales, raw
 * quaternions, opacity logits, features_dc [N,1,3], features_rest [N,k-1,3]; no scene graph).  Row b*N + i of every
 * per-row array is Gaussian i seen from camera b; images are [B,H,W,C].  Every output of view b is bit-identical to the
 * single-view fused path for camera b alone (same kernel bodies, local pixel coordinates); gradients w.r.t. the N
 * Gaussians are sums over the views, summed in registers in ascending view order (projection, SH, opacity: no float
 * atomics) — the raster backward keeps its atomics.
 * `cams`: HOST array of n_views rows; it is copied into the kernel arguments (no device buffer).
 * Return codes of every entry below: -1 n_views outside [1, SGN_VIEWS_MAX]; -2 n < 0 or n_views * n >= 2^28 (sorted ids
 * carry quadrant masks in bits 28-31); -3 bad image size / block width (the raster entries need block_width 16); -4 a
 * required pointer is NULL; -5 workspace / arena too small; -6 isect_capacity < 1 or >= 2^31; SGN_E_CAPACITY as
 * sgn_rasterize_fwd_all. */
#define SGN_VIEWS_MAX 16
typedef struct sgn_view_cam {
    float viewmat[12];  /* world -> camera, 3x4 row-major */
    float fx, fy, cx, cy;
    float cam_pos[3];   /* camera centre in world coordinates (SH view directions) */
} sgn_view_cam;

/* Projection: outputs [n_views * n, ...] as sgn_project_fwd_fused per camera (no object ids / poses). */
int sgn_project_views_fwd(int n_views, int n, const sgn_view_cam *cams, const float *means, const float *log_scales,
                          float glob_scale, const float *quats_raw, int img_h, int img_w, int block_width,
                          float clip_thresh, float *cov3d, float *xys, float *depths, int32_t *radii, float *conics,
                          float *compensation, int32_t *num_tiles_hit, int semantics, sgn_stream_t stream);
/* Its backward: v_* [n_views * n, ...] in, gradients w.r.t. the n Gaussians out (summed over the views). */
int sgn_project_views_bwd(int n_views, int n, const sgn_view_cam *cams, const float *means, const float *log_scales,
                          float glob_scale, const float *quats_raw, const float *cov3d, const int32_t *radii,
                          const float *conics, const float *compensation, const float *v_xy, const float *v_depth,
                          const float *v_conic, const float *v_compensation, float *v_means, float *v_log_scales,
                          float *v_quats_raw, int semantics, int img_h, int img_w, sgn_stream_t stream);

/* SH colours of every view, clamp(SH + 0.5, min 0) (post_half_clamp) as sgn_sh_fwd_fused with n_fourier = 1: the
 * coefficients are read once, colors [n_views * n, 3].  The backward sums the views' coefficient gradients. */
int sgn_sh_views_fwd(int n_views, int n, int k, int degree, const sgn_view_cam *cams, const float *means,
                     const float *features_dc, const float *features_rest, int post_half_clamp, float *colors,
                     sgn_stream_t stream);
int sgn_sh_views_bwd(int n_views, int n, int k, int degree, const sgn_view_cam *cams, const float *means,
                     int post_half_clamp, const float *colors, const float *v_colors, float *v_features_dc,
                     float *v_features_rest, sgn_stream_t stream);

/* The forward of the batched rasterization in ONE call, as sgn_rasterize_fwd_all over all views: the depth ranking of
 * all n_views * n rows, the per-row tile counts on each view's own grid, ONE host wait for the intersection count, the
 * rows, the emission with tile id = view * tiles_per_view + local tile (each tile's list then holds its own view's rows
 * in depth order), the tile sort, the launch order over all tiles and the forward kernels.  opacity_logits [n] (row
 * b*n+i reads entry i); out_img [B,H,W,3], final_Ts / final_idx / out_depth (NULL: no depth channel) [B,H,W];
 * tile_bins and tile_stats [B*tiles, 2] (tile_stats right behind tile_bins saves a clear), tile_order [B*tiles + 2],
 * rows: sgn_raster_workspace_bytes(n_views * n).  Returns 0 with *n_isect_host = 0 when nothing is visible (the
 * images are not written). */
size_t sgn_rasterize_views_arena_bytes(int n_views, int n, int64_t isect_capacity);
int sgn_rasterize_views_fwd_all(int n_views, int n, const float *xys, const float *depths, const int32_t *radii,
                                const float *conics, const float *colors, const float *opacity_logits, int cull,
                                int img_h, int img_w, int block_width, const float *background3, int quadrant_masks,
                                float *out_img, float *final_Ts, int32_t *final_idx, float *out_depth,
                                int32_t *gaussian_ids_sorted, int64_t isect_capacity, int32_t *tile_bins,
                                int32_t *tile_order, int32_t *tile_stats, void *rows, size_t rows_bytes,
                                void *order_scratch, size_t order_scratch_bytes, void *arena, size_t arena_bytes,
                                int32_t *count_pinned, int64_t *n_isect_host, int sort_rank_mode, int semantics,
                                const sgn_raster_opts *opts, sgn_stream_t stream);
/* Its backward: launch order from the forward's tile statistics, the reverse walks of every view's tiles (gradient
 * atomics into grad_ws, sgn_raster_bwd_workspace_bytes(n_views * n)), then one pass that unpacks v_xy / v_conic /
 * v_colors [n_views * n, ...] and sums d/d logit over the views into v_opacity_logits [n]. */
int sgn_rasterize_views_bwd_all(int n_views, int n, int64_t n_isect, int img_h, int img_w,
                                const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const int32_t *tile_stats,
                                const float *conics, const float *opacity_logits, const float *background3,
                                const float *final_Ts, const int32_t *final_idx, const float *v_out_img,
                                const float *v_out_alpha, float alpha_clamp_bwd, float *v_xy, float *v_conic,
                                float *v_colors, float *v_opacity_logits, const void *rows, size_t rows_bytes,
                                void *grad_ws, size_t grad_ws_bytes, int32_t *tile_order, void *order_scratch,
                                size_t order_scratch_bytes, int small_q16, const sgn_raster_opts *opts,
                                sgn_stream_t stream, sgn_stream_t aux_stream);

#ifdef __cplusplus
}
#endif
#endif /* SGN_RAST_H */
