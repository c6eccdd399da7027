// raster_absgrad.hip — the reverse walk with the absgrad statistic (AbsGS; gsplat's `absgrad=True` / `means2d.absgrad`):
// besides everything raster.hip's backward computes, per Gaussian the sum over the pixels it was composited onto of the
// ABSOLUTE screen-space gradient, v_xy_abs = sum_pixels |dL/d xy|.  Densification that decides from the norm of the
// signed v_xy misses large splats over fine texture, whose per-pixel gradients point in opposing directions and cancel.
//
// The per-pixel gradient exists only inside the walk: raster_bwd_tile (raster_common.h) reduces raw moments and the conic
// is applied once per Gaussian afterwards, and an absolute value does not commute with that.  So the body is the same
// one, instantiated with ABSGRAD = true: per evaluated (pixel, entry) pair, after p = vs*dx, q = vs*dy,
//   ax += fabsf(fmaf(A, p, b * q)),  ay += fabsf(fmaf(b, p, C * q)),   A = ha + ha, C = hc + hc (once per entry)
// (the contract is stated with the body).  ax, ay ride the wave reduction — lanes 9, 10 of the butterfly form, the spare
// rows of the third register of the swap form: one more swap per reduction — into slots 9, 10 of the Gaussian's row of
// the packed gradient workspace, which the plain kernels leave at zero.
//
// Its own translation unit, built with raster.hip's flags (-ffp-contract=off -fno-slp-vectorize): raster.hip's set of
// kernels, their registers and their swap counts are pinned by tests/test_isa_properties.py and stay what they were;
// what is off by default costs the default nothing, not even code size in the unit the benchmark runs.
//
// The three launch shapes of the plain backward (raster.hip "Launch shapes of the backward"), each exact x reduce.
#include "sgn_common.h"
#include "raster_common.h"

namespace {

template <bool EXACT, int REDUCE, int QPW, bool ADAPT, int MODE>
__global__ __launch_bounds__(64) void raster_absbwd_kernel(int W, int H, int B, int tiles_x, int n_tiles,
                                                           const int2 *__restrict__ bins,
                                                           const Rec *__restrict__ recs,
                                                           const int32_t *__restrict__ ids,
                                                           const float *__restrict__ bg,
                                                           const float *__restrict__ final_T,
                                                           const int32_t *__restrict__ final_idx,
                                                           const float *__restrict__ v_out,
                                                           const float *__restrict__ v_out_alpha,
                                                           float alpha_clamp, float *__restrict__ grad_ws, int dbg,
                                                           int adapt_thresh, int batch_thresh,
                                                           const int32_t *__restrict__ tile_order, int use_qm) {
    if constexpr (MODE == 0) {
        static_assert(QPW == 4 && ADAPT, "MODE 0 is the in-kernel adaptive split");
        int tile = (int)(blockIdx.x % n_tiles);      // wave-major numbering, as raster_bwd_kernel
        if (tile_order) tile = tile_order[tile];
        const int wv = (int)(blockIdx.x / n_tiles);
        raster_bwd_tile<EXACT, REDUCE, QPW, ADAPT, true>(tile, wv, W, H, B, tiles_x, bins, recs, ids, bg, final_T,
                                                         final_idx, v_out, v_out_alpha, alpha_clamp, grad_ws, dbg,
                                                         adapt_thresh, batch_thresh, use_qm);
    } else {
        static_assert(MODE == 2, "MODE 1 lives in raster_absbwd_short_kernel");
        static_assert(QPW == 1 && !ADAPT, "long tiles: four lean waves per tile");
        if ((int)blockIdx.x >= 4 * tile_order[n_tiles]) return;
        __builtin_amdgcn_s_setprio(3);               // the critical path on skewed content, as in raster_bwd_kernel
        raster_bwd_tile<EXACT, REDUCE, 1, false, true>(tile_order[blockIdx.x >> 2], blockIdx.x & 3, W, H, B, tiles_x,
                                                       bins, recs, ids, bg, final_T, final_idx, v_out, v_out_alpha,
                                                       alpha_clamp, grad_ws, dbg, adapt_thresh, batch_thresh, use_qm);
    }
}

// the short-walk half, held at four waves per SIMD like raster_bwd_short_kernel (it shares the SIMDs with the long-walk
// kernel, which is the critical path)
template <bool EXACT, int REDUCE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void raster_absbwd_short_kernel(
    int W, int H, int B, int tiles_x, int n_tiles, const int2 *__restrict__ bins, const Rec *__restrict__ recs,
    const int32_t *__restrict__ ids, const float *__restrict__ bg, const float *__restrict__ final_T,
    const int32_t *__restrict__ final_idx, const float *__restrict__ v_out, const float *__restrict__ v_out_alpha,
    float alpha_clamp, float *__restrict__ grad_ws, int dbg, int adapt_thresh, int batch_thresh,
    const int32_t *__restrict__ tile_order, int use_qm) {
    const int n_long = tile_order[n_tiles];
    if ((int)blockIdx.x < n_long) return;
    raster_bwd_tile<EXACT, REDUCE, 4, false, true>(tile_order[blockIdx.x], 0, W, H, B, tiles_x, bins, recs, ids, bg,
                                                   final_T, final_idx, v_out, v_out_alpha, alpha_clamp, grad_ws, dbg,
                                                   adapt_thresh, batch_thresh, use_qm);
}

// unpack_grads_kernel (raster.hip) for the n rows of a whole-tensor pass, plus v_xy_abs[i] = (ws[9], ws[10])
__global__ __launch_bounds__(256) void unpack_grads_abs_kernel(int n, const float *__restrict__ ws,
                                                               const float *__restrict__ conics,
                                                               const float *__restrict__ opac, int opac_is_logit,
                                                               const float *__restrict__ colors_pre,
                                                               float *__restrict__ v_xy, float *__restrict__ v_conic,
                                                               float *__restrict__ v_colors,
                                                               float *__restrict__ v_opac,
                                                               float *__restrict__ v_xy_abs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 a = reinterpret_cast<const float4 *>(ws)[3 * (size_t)i + 0];
    const float4 b = reinterpret_cast<const float4 *>(ws)[3 * (size_t)i + 1];
    const float4 c = reinterpret_cast<const float4 *>(ws)[3 * (size_t)i + 2];
    unpack_row(i, a, b, c, conics, opac, opac_is_logit, colors_pre, v_xy, v_conic, v_colors, v_opac);
    v_xy_abs[2 * i] = c.y;
    v_xy_abs[2 * i + 1] = c.z;
}

// this unit's backward family for sgn_raster_bwd_launch (raster_common.h), [exact_exp][reduce_mode]
const RasterBwdFamily absbwd_family = {
    {{raster_absbwd_kernel<false, 0, 4, true, 0>, raster_absbwd_kernel<false, 1, 4, true, 0>},
     {raster_absbwd_kernel<true, 0, 4, true, 0>, raster_absbwd_kernel<true, 1, 4, true, 0>}},
    {{raster_absbwd_kernel<false, 0, 1, false, 2>, raster_absbwd_kernel<false, 1, 1, false, 2>},
     {raster_absbwd_kernel<true, 0, 1, false, 2>, raster_absbwd_kernel<true, 1, 1, false, 2>}},
    {{raster_absbwd_short_kernel<false, 0>, raster_absbwd_short_kernel<false, 1>},
     {raster_absbwd_short_kernel<true, 0>, raster_absbwd_short_kernel<true, 1>}}};

}  // namespace

// sgn_raster_bwd_part with the absgrad statistic (include/sgn_rast.h).
SGN_EXPORT int sgn_raster_bwd_abs(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                                  const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                                  const float *conics, const float *colors, const float *opacities,
                                  int opacity_is_logit, int id_lo, int id_hi, int window, const float *background3,
                                  const float *final_Ts, const int32_t *final_idx, const float *v_out_img,
                                  const float *v_out_alpha, float alpha_clamp_bwd, float *v_xy, float *v_conic,
                                  float *v_colors, float *v_opacity, void *recs_ws, size_t recs_ws_bytes,
                                  int recs_packed, void *grad_ws, size_t grad_ws_bytes, const int32_t *tile_order,
                                  const float *colors_pre_clamp, const sgn_raster_opts *opts, sgn_stream_t stream,
                                  sgn_stream_t aux_stream, int first, int last, float *v_xy_abs) {
    SGN_ARG_CHECK(!window, -13);
    SGN_ARG_CHECK(v_xy_abs != nullptr, -14);
    // this entry holds the id range to its bounds without a window too (the shared checks: under a window only), at its
    // place in their order
    SGN_ARG_CHECK(opacity_is_logit >= 0 && opacity_is_logit <= 2, -11);
    SGN_ARG_CHECK(0 <= id_lo && id_lo <= id_hi && id_hi <= n, -9);
    const RasterBwdCall c = {img_h, img_w, block_width, n, n_isect, gaussian_ids_sorted, tile_bins, xys, conics, colors,
                             opacities, opacity_is_logit, id_lo, id_hi, window, background3, final_Ts, final_idx,
                             v_out_img, v_out_alpha, alpha_clamp_bwd, v_xy, v_conic, v_colors, v_opacity, recs_ws,
                             recs_ws_bytes, recs_packed, grad_ws, grad_ws_bytes, tile_order, colors_pre_clamp, opts,
                             stream, aux_stream};
    const int rc = sgn_raster_bwd_walks(__func__, &absbwd_family, &c, first);
    if (rc != 0 || n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    sgn_timing_begin(SGN_T_UNPACK, s);
    if (last)
        hipLaunchKernelGGL(unpack_grads_abs_kernel, dim3(sgn_cdiv(n, 256)), dim3(256), 0, s, n, (const float *)grad_ws,
                           conics, opacities, opacity_is_logit, colors_pre_clamp, v_xy, v_conic, v_colors, v_opacity,
                           v_xy_abs);
    sgn_timing_end(SGN_T_UNPACK, s);
    SGN_LAUNCH_CHECK();
    return 0;
}
