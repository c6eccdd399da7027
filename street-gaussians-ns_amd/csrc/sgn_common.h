// Internal helpers shared by the HIP translation units of libsgnrast.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "sgn_rast.h"

#define SGN_EXPORT extern "C" __attribute__((visibility("default")))

void sgn_set_error(const char *fmt, ...);
int sgn_timing_enabled();
void sgn_timing_begin(int slot, void *stream);
void sgn_timing_end(int slot, void *stream);
int sgn_fork_events(hipEvent_t *fork, hipEvent_t *join);   // api.cpp: cached per (thread, device)

// SGN_ARG_CHECK_FN: the message carries `fn` — checks shared by several entries are handed the public entry's name.
// (`text` is stringized where the condition is written, before its macros such as HALO expand.)
#define SGN_ARG_CHECK_TEXT_(fn, cond, text, code)                              \
    do {                                                                       \
        if (!(cond)) {                                                         \
            sgn_set_error("%s: argument check failed: %s", (fn), text);        \
            return (code);                                                     \
        }                                                                      \
    } while (0)
#define SGN_ARG_CHECK_FN(fn, cond, code) SGN_ARG_CHECK_TEXT_(fn, cond, #cond, code)
#define SGN_ARG_CHECK(cond, code) SGN_ARG_CHECK_TEXT_(__func__, cond, #cond, code)

#define SGN_HIP_CHECK(expr)                                                    \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) {                                                \
            sgn_set_error("%s: %s -> %s", __func__, #expr, hipGetErrorString(e_)); \
            return (int)e_;                                                    \
        }                                                                      \
    } while (0)

#define SGN_LAUNCH_CHECK()                                                     \
    do {                                                                       \
        hipError_t e_ = hipGetLastError();                                     \
        if (e_ != hipSuccess) {                                                \
            sgn_set_error("%s: launch failed: %s", __func__, hipGetErrorString(e_)); \
            return (int)e_;                                                    \
        }                                                                      \
    } while (0)

// ---- internal entry points that api.cpp's one-call entries are built from (not part of include/sgn_rast.h)
// project.hip: sgn_project_fwd with upstream's unit-quaternion assertion riding the kernel (quat_flag nullptr: none); a
// failing row stores quat_stamp into *quat_flag, and — quat_ok != nullptr — the kernel's first lane stores it into
// *quat_ok ("this launch's stores land where the host looks"); both system-scope
int sgn_project_fwd_checked(int n, const float *means3d, const float *scales, float glob_scale, const float *quats,
                            const float *viewmat12, float fx, float fy, float cx, float cy, int img_h, int img_w,
                            int block_width, float clip_thresh, float *cov3d, float *xys, float *depths, int32_t *radii,
                            float *conics, float *compensation, int32_t *num_tiles_hit, int32_t *quat_flag,
                            float quat_tol, int32_t quat_stamp, int32_t *quat_ok, int semantics, sgn_stream_t stream);
// project.hip: one wave copies n words (<= 64) into mapped pinned memory, then stores flag_value into *flag_mapped
int sgn_publish_words(const int32_t *src_dev, int n, int32_t *dst_mapped, int32_t *flag_mapped, int32_t flag_value,
                      sgn_stream_t stream);
// binning.hip: sgn_bin_prepare; `total_host`: device-visible pointer into pinned host memory (or nullptr) that receives
// cum_by_rank[n-1] from the scan itself, `extra_dev` -> `extra_host` one more word stored ahead of it
int sgn_bin_prepare_total(int n, const float *xys, const float *depths, const int32_t *radii,
                          const float *conics, const float *opacities, int opacity_is_logit, int cull,
                          int tiles_x, int tiles_y, int block_width, int32_t *cum_by_rank,
                          int32_t *gid_by_rank, int rank_ready, float *bin_records, void *ws, size_t ws_bytes,
                          int sort_rank_mode, int32_t *total_host, const int32_t *extra_dev, int32_t *extra_host,
                          int semantics, sgn_stream_t stream);
// binning.hip: sgn_bin_intersect; `also_zero_words`: int32 words BEHIND tile_bins' 2 * n_tiles that the emission clears
// as well (the one-call forward puts the raster kernels' tile statistics there: a clear that needs no launch of its own)
int sgn_bin_intersect_zero(int n, int64_t n_isect, const float *bin_records, const int32_t *cum_by_rank,
                           const int32_t *gid_by_rank, int tiles_x, int tiles_y, int block_width,
                           int32_t *gaussian_ids_sorted, int32_t *tile_bins, int quadrant_masks, void *ws,
                           size_t ws_bytes, const int32_t *n_isect_dev, int sort_rank_mode, int also_zero_words,
                           sgn_stream_t stream);
// binning.hip: the same over n = n_views * n_per_view rows of one depth ranking, 16x16 tiles
int sgn_bin_intersect_views(int n_views, int n, int64_t n_isect, const float *bin_records, const int32_t *cum_by_rank,
                            const int32_t *gid_by_rank, int tiles_x, int tiles_y, int32_t *gaussian_ids_sorted,
                            int32_t *tile_bins, int quadrant_masks, void *ws, size_t ws_bytes,
                            const int32_t *n_isect_dev, int sort_rank_mode, int also_zero_words, sgn_stream_t stream);
// raster.hip: sgn_raster_fwd (full scene, rows built) behind a launch that already cleared tile_kmax
int sgn_raster_fwd_precleared(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                              const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                              const float *conics, const float *colors, const float *opacities,
                              int opacity_is_logit, const float *background3, float *out_img, float *final_Ts,
                              int32_t *final_idx, void *recs_ws, size_t recs_ws_bytes, const int32_t *tile_order,
                              int32_t *tile_kmax, const float *depths, float *out_depth, const sgn_raster_opts *opts,
                              sgn_stream_t stream);
// raster.hip: host side of the batched views' raster passes
int sgn_views_repeat(int n, int n_views, const float *src, float *dst, sgn_stream_t stream);
int sgn_raster_views_fwd(int n_views, int img_h, int img_w, const int32_t *ids, const int32_t *tile_bins,
                         const void *rows, const float *background3, float *out_img, float *final_Ts,
                         int32_t *final_idx, const int32_t *tile_order, int32_t *tile_kmax, const float *depths,
                         float *out_depth, const sgn_raster_opts *opts, sgn_stream_t stream);
int sgn_raster_views_bwd(int n_views, int n, int img_h, int img_w, const int32_t *ids, const int32_t *tile_bins,
                         const void *rows, const float *conics, const float *logits, const float *background3,
                         const float *final_Ts, const int32_t *final_idx, const float *v_out_img,
                         const float *v_out_alpha, float alpha_clamp_bwd, float *v_xy, float *v_conic, float *v_colors,
                         float *v_opacity, void *grad_ws, const int32_t *tile_order, const sgn_raster_opts *opts,
                         sgn_stream_t stream, sgn_stream_t aux_stream);

// gt_pyramid.hip: the launch behind sgn_gt_downscale (api.cpp checks the arguments); the two fp32 quotients in / out are
// formed on the host and travel as kernel arguments
int sgn_gt_downscale_launch(int h, int w, int oh, int ow, const unsigned char *image, const unsigned char *mask,
                            const unsigned char *semantic, float *image_out, unsigned char *mask_out,
                            unsigned char *semantic_out, sgn_stream_t stream);

// frame_pack.hip: the launch behind sgn_frames_pack (api.cpp checks the arguments); the panel table is copied into the
// kernel arguments
int sgn_frames_pack_launch(int h, int w, int n_panels, const sgn_panel *panels, unsigned char *canvas, int canvas_w,
                           sgn_stream_t stream);

// bilagrid.hip: the launches behind sgn_bilagrid_slice_fwd / _bwd (api.cpp checks the arguments)
int sgn_bilagrid_slice_fwd_launch(int L, int Hg, int Wg, const float *grid, int H, int W, int n_pix, const float *rgb,
                                  float *out, sgn_stream_t stream);
int sgn_bilagrid_slice_bwd_launch(int L, int Hg, int Wg, const float *grid, int H, int W, int n_pix, const float *rgb,
                                  const float *v_out, float *v_rgb, float *v_grid, sgn_stream_t stream);

// Batched views (include/sgn_rast.h "Batched views"): the camera table travels BY VALUE as a kernel argument (SGPRs /
// the kernarg segment, no device buffer, no copy), one entry per view; the host fills it from sgn_view_cam rows.
struct SgnViews {
    int n;                                  // views, 1..SGN_VIEWS_MAX
    float V[SGN_VIEWS_MAX][12];             // world -> camera, 3x4 row-major
    float fx[SGN_VIEWS_MAX], fy[SGN_VIEWS_MAX], cx[SGN_VIEWS_MAX], cy[SGN_VIEWS_MAX];
    float lim_x[SGN_VIEWS_MAX], lim_y[SGN_VIEWS_MAX];   // 1.3 tan(fov / 2) of the projection's clamp
    float pos[SGN_VIEWS_MAX][3];            // camera centre (SH view directions)
};
// argument checks shared by the batched entries: 1 <= n_views <= SGN_VIEWS_MAX, n >= 0 and n_views * n < 2^28 (sorted
// ids carry quadrant masks in bits 28-31)
static inline bool sgn_views_rows_ok(int n_views, int n) {
    return n >= 0 && (int64_t)n_views * (int64_t)n < ((int64_t)1 << 28);
}
static inline SgnViews sgn_views_table(int n_views, const sgn_view_cam *cams, int img_h, int img_w, bool lim_from_image) {
    SgnViews t = {};
    t.n = n_views;
    for (int b = 0; b < n_views; ++b) {
        const sgn_view_cam &c = cams[b];
        for (int k = 0; k < 12; ++k) t.V[b][k] = c.viewmat[k];
        t.fx[b] = c.fx; t.fy[b] = c.fy; t.cx[b] = c.cx; t.cy[b] = c.cy;
        // as project.hip make_cam / bwd_cam: the backward needs the image's clamp only for SGN_SEM_EWA_VJP_CLAMPED
        const int w = lim_from_image ? img_w : 16, h = lim_from_image ? img_h : 16;
        t.lim_x[b] = 1.3f * (0.5f * (float)w / c.fx);
        t.lim_y[b] = 1.3f * (0.5f * (float)h / c.fy);
        for (int k = 0; k < 3; ++k) t.pos[b][k] = c.cam_pos[k];
    }
    return t;
}

static inline int sgn_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// A byte of a cached uint8 image as the fp32 it stands for: the correctly rounded quotient u / 255 (IEEE division, NOT
// u * (1 / 255): 126 of the 256 byte values differ in the last bit).  Shared by the byte loss (loss.hip) and the
// ground-truth pyramid (gt_pyramid.hip), which therefore form the same number.
__device__ __forceinline__ float sgn_byte_unorm(unsigned char u) { return __fdiv_rn((float)u, 255.f); }

// float -> int with v_cvt_i32_f32 semantics (saturating, NaN -> 0); the C oracle spells the
// same rule out (oracle/c/sgn_oracle.c f2i).
__device__ __forceinline__ int sgn_f2i(float v) {
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return (-2147483647 - 1);
    return (int)v;
}

// gsplat helpers.cuh get_tile_bbox / get_bbox: inclusive min, exclusive max.
// `semantics` & SGN_SEM_BBOX_ADD_AFTER_CAST: the max side is (int)(c + r) + 1 (gsplat/_torch_impl.py) instead of the
// default (int)(c + r + 1) (gsplat helpers.cuh); include/sgn_rast.h "upstream-variant semantics".
__device__ __forceinline__ int sgn_bbox_max(float v, int semantics) {
    if (semantics & SGN_SEM_BBOX_ADD_AFTER_CAST) {
        const int t = sgn_f2i(v);
        return t == 2147483647 ? t : t + 1;
    }
    return sgn_f2i(v + 1.0f);
}
__device__ __forceinline__ void sgn_tile_bbox(float cx, float cy, float radius, int tiles_x,
                                              int tiles_y, int block, int &mnx, int &mny, int &mxx,
                                              int &mxy, int semantics = 0) {
    const float fb = (float)block;
    const float tcx = cx / fb, tcy = cy / fb, tr = radius / fb;
    mnx = min(max(0, sgn_f2i(tcx - tr)), tiles_x);
    mxx = min(max(0, sgn_bbox_max(tcx + tr, semantics)), tiles_x);
    mny = min(max(0, sgn_f2i(tcy - tr)), tiles_y);
    mxy = min(max(0, sgn_bbox_max(tcy + tr, semantics)), tiles_y);
}
