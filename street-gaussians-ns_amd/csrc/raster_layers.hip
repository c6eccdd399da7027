// raster_layers.hip — forward-only "layered" compositing for evaluation renders, gfx950.
//
// The scene graph's evaluation outputs (sgn_splatfacto_scene_graph.py:363-372 with self.training == False) are six
// rasterizations of one depth list in the reference: rgb + alpha, depth, objects-only accumulation, background-only
// accumulation, background-only rgb, objects-only rgb.  This kernel walks a tile's list ONCE and composites three layers
// per pixel:
//   all   every entry          C0..C2, the depth channel D, T
//   head  ids <  split         C0..C2, T        (the background sub-model)
//   tail  ids >= split         C0..C2, T        (the objects)
// sigma / alpha / the alpha >= 1/255, sigma >= 0 and nT <= 1e-4 tests are those of raster.hip's raster_fwd_tile (same
// operations, same order: the arithmetic contract of that file's header) and are evaluated once per (entry, pixel); each
// layer the entry belongs to then runs the single pass's `vis = alpha T; C = fma(c, vis, C); T = nT` recursion on its own
// state, so every layer is BIT-EQUAL to sgn_raster_fwd over that id range (tests/test_gpu_layers.py).  There is no
// backward, hence no final index, no per-tile walk depth and no group index spaces.
//
// Shape of the launch: that of the packed forward — the first tile_order[n_tiles] tiles of the launch order (the longest
// lists) get four waves, one 8x8 quadrant each, the others two waves with a 16x8 half each — and the same two ways
// through a list (scalar chase one entry ahead; 64-entry batches staged in wave-private LDS from batch_fwd entries on:
// raster_common.h's walk_chase / walk_staged and its packed_launch_map, the very source the packed forward runs).
// The walk of the shared list goes on while the all-layer or the head layer is alive.  The tail layer — a few objects
// in front of a saturated background never finish — goes on along ITS OWN compacted list (sgn_list_window) from where
// the shared walk left it, as the GROUPS forward does; without such a list it keeps the shared walk alive instead.
// A tile that holds no tail entry (most of the image), or a scene with an empty head / tail range, runs the plain
// one-layer walk and copies: the other non-empty layer IS the all-layer there.
#include "sgn_common.h"
#include "raster_common.h"

namespace {

struct LayerArgs {
    int W, H, tiles_x, n_tiles;
    int split, n;               // head: ids < split; tail: ids >= split
    int batch_thresh, use_qm;
    const int2 *bins;           // shared list
    const int32_t *ids;
    const int2 *own_bins;       // the tail layer's own compacted list (nullptr: none)
    const int32_t *own_ids;
    const Rec *recs;
    const float *depths;
    const float *bg;
    const int32_t *tile_order;
    float *out_img;             // [3][H*W*3]  all, head, tail
    float *final_T;             // [3][H*W]
    float *out_depth;           // [H*W]
};

// MODE 0: three layers.  MODE 1: the all-layer alone (the caller copies it to the layer it equals).
template <bool EXACT, int QPW, int MODE>
__device__ __forceinline__ void layers_tile(const LayerArgs &A, int tile, int wv, float4 (*stage)[64 * 3],
                                            float (*stage_d)[64], int copy_to) {
    constexpr bool LAYERS = MODE == 0;
    const int lane = threadIdx.x;
    const int2 range = A.bins[tile];
    const bool qm_on = A.use_qm != 0;
    const int idmask = qm_idmask(A.use_qm);
    const int q0 = wv * QPW;
    const int tx = tile % A.tiles_x, ty = tile / A.tiles_x;
    const float bg0 = A.bg[0], bg1 = A.bg[1], bg2 = A.bg[2];
    const int W = A.W, H = A.H, split = A.split;
    const bool own = LAYERS && A.own_bins != nullptr;   // the tail layer finishes on its own list

    // "finished (or outside the image)" is the SIGN of T, per layer (raster.hip)
    float px[QPW], py[QPW], T[QPW], C0[QPW], C1[QPW], C2[QPW], Dq[QPW];
    float TH[LAYERS ? QPW : 1], H0[LAYERS ? QPW : 1], H1[LAYERS ? QPW : 1], H2[LAYERS ? QPW : 1];
    float TT[LAYERS ? QPW : 1], L0[LAYERS ? QPW : 1], L1[LAYERS ? QPW : 1], L2[LAYERS ? QPW : 1];
    int pix[QPW];
    bool inside[QPW];
#pragma unroll
    for (int q = 0; q < QPW; ++q) {
        const int ox = ((q0 + q) & 1) * 8 + (lane & 7), oy = ((q0 + q) >> 1) * 8 + (lane >> 3);
        const int j = tx * 16 + ox, i = ty * 16 + oy;
        inside[q] = j < W && i < H;
        pix[q] = i * W + j;
        px[q] = (float)j + 0.5f;
        py[q] = (float)i + 0.5f;
        T[q] = inside[q] ? 1.f : -1.f;
        C0[q] = C1[q] = C2[q] = Dq[q] = 0.f;
    }
    if constexpr (LAYERS) {
#pragma unroll
        for (int q = 0; q < QPW; ++q) {
            TH[q] = TT[q] = T[q];
            H0[q] = H1[q] = H2[q] = L0[q] = L1[q] = L2[q] = 0.f;
        }
    }
    const float qcx = (float)(tx * 16 + (lane & 1) * 8) + 4.0f, qcy = (float)(ty * 16 + ((lane >> 1) & 1) * 8) + 4.0f;

    // one entry for this wave's pixels.  `tail`: the entry's layer besides the all-layer (wave-uniform); `own_walk`:
    // the tail layer's walk of the rest of its own list (the all-layer takes no part).  false: nothing left to do.
    auto entry = [&](const Rec &cur, unsigned qm, float dep, bool tail, bool own_walk) __attribute__((always_inline)) -> bool {
        unsigned long long live[QPW], liveg[QPW], keep = 0ull;
#pragma unroll
        for (int q = 0; q < QPW; ++q) {
            live[q] = __ballot(T[q] > 0.f);
            liveg[q] = 0ull;
            if constexpr (LAYERS) {
                liveg[q] = __ballot((tail ? TT[q] : TH[q]) > 0.f);
                if (own_walk) { live[q] = 0ull; keep |= liveg[q]; }
                // the all-layer cannot outlive both others; a tail layer with its own list does not hold the shared walk
                else keep |= live[q] | __ballot(TH[q] > 0.f || (!own && TT[q] > 0.f));
            } else {
                keep |= live[q];
            }
        }
        if (keep == 0ull) return false;
#pragma unroll
        for (int q = 0; q < QPW; ++q) {
            if ((live[q] | liveg[q]) == 0ull || !((qm >> (q0 + q)) & 1u)) continue;  // wave-uniform
            const float dx = cur.x - px[q], dy = cur.y - py[q];
            float s = (cur.ha * dx) * dx;
            s = fmaf(cur.hc * dy, dy, s);
            const float sigma = fmaf(cur.b * dx, dy, s);
            const float alpha = fminf(0.999f, cur.opac * sgn_exp<EXACT>(-sigma));
            const bool ok = sigma >= 0.f && alpha >= (1.f / 255.f);
            if (!(LAYERS && own_walk)) {
                const bool valid = T[q] > 0.f && ok;
                const float nT = T[q] * (1.f - alpha);
                const bool stop = valid && nT <= 1e-4f;
                const bool acc = valid && !stop;
                const float vis = acc ? alpha * T[q] : 0.f;
                C0[q] = fmaf(cur.r, vis, C0[q]);
                C1[q] = fmaf(cur.g, vis, C1[q]);
                C2[q] = fmaf(cur.bl, vis, C2[q]);
                Dq[q] = fmaf(dep, vis, Dq[q]);
                const float Tk = acc ? nT : T[q];
                T[q] = stop ? -Tk : Tk;   // the terminating entry is not composited; T keeps its last value
            }
            if constexpr (LAYERS) {
                const float Tg = tail ? TT[q] : TH[q];
                const bool valid = Tg > 0.f && ok;
                const float nT = Tg * (1.f - alpha);
                const bool stop = valid && nT <= 1e-4f;
                const bool acc = valid && !stop;
                const float vis = acc ? alpha * Tg : 0.f;
                const float Tk = acc ? nT : Tg;
                const float Tn = stop ? -Tk : Tk;
                if (tail) {
                    L0[q] = fmaf(cur.r, vis, L0[q]); L1[q] = fmaf(cur.g, vis, L1[q]); L2[q] = fmaf(cur.bl, vis, L2[q]);
                    TT[q] = Tn;
                } else {
                    H0[q] = fmaf(cur.r, vis, H0[q]); H1[q] = fmaf(cur.g, vis, H1[q]); H2[q] = fmaf(cur.bl, vis, H2[q]);
                    TH[q] = Tn;
                }
            }
        }
        return true;
    };

    int cO = 0;      // tail entries of the shared list met so far
    int rO = -1;     // ... when the shared walk stopped early (-1: it reached the end of the list)
    auto box_mask = [&](int raw, const Rec &cur) __attribute__((always_inline)) -> unsigned {
        return qm_on ? qm_bits(raw, cur.ex) : quadrant_mask(cur, qcx, qcy, true);
    };
    const int L = range.y - range.x;
    if (L < A.batch_thresh) {
        walk_chase<1, true>(A.ids, A.recs, A.depths, idmask, range.x, range.y - 1, [&](const Rec &cur, int raw, int, float dep) {
            const bool tail = LAYERS && (raw & idmask) >= split;
            if (!entry(cur, box_mask(raw, cur), dep, tail, false)) { rO = cO; return false; }   // this entry is still to come
            cO += (int)tail;
            return true;
        });
    } else {
        unsigned mine_q = 0u;
#pragma unroll
        for (int q = 0; q < QPW; ++q) mine_q |= 1u << (q0 + q);
        unsigned long long tmask = 0ull;   // the batch's tail entries
        int cB = 0;                        // tail entries before the batch
        walk_staged<1, true>(
            A.ids, A.recs, A.depths, idmask, range.x, L, stage, stage_d,
            [&](int raw, const float4 &r0, const float4 &r2) {
                return (qm_on ? qm_bits(raw, r2.z) : row_quadrants(r0.x, r0.y, r2.z, r2.w, tx * 16, ty * 16, true)) & mine_q;
            },
            [&](bool in_batch, int raw) {
                if constexpr (LAYERS) {
                    tmask = __ballot(in_batch && (raw & idmask) >= split);
                    cB = cO;
                    cO += __popcll(tmask);
                }
            },
            [&](const Rec &cur, int j, int, unsigned qm, float dep) {
                if (entry(cur, qm, dep, (tmask >> j) & 1ull, false)) return true;
                rO = cB + __popcll(tmask & ((1ull << j) - 1ull));
                return false;
            });
    }
    if constexpr (LAYERS) {
        if (own) {
            // the tail layer outlived the shared walk: the rest of its own list
            const int2 ob = A.own_bins[tile];
            const int from = ob.x + (rO < 0 ? cO : rO);
            walk_chase<1, false>(A.own_ids, A.recs, nullptr, idmask, from, ob.y - 1, [&](const Rec &cur, int raw, int, float) {
                return entry(cur, box_mask(raw, cur), 0.f, true, true);
            });
        }
    }
    const size_t HW = (size_t)W * (size_t)H;
#pragma unroll
    for (int q = 0; q < QPW; ++q) {
        if (!inside[q]) continue;
        const size_t p = (size_t)pix[q];
        const float Ta = fabsf(T[q]);
        const float a0 = fmaf(Ta, bg0, C0[q]), a1 = fmaf(Ta, bg1, C1[q]), a2 = fmaf(Ta, bg2, C2[q]);
        A.final_T[p] = Ta;
        A.out_img[3 * p + 0] = a0; A.out_img[3 * p + 1] = a1; A.out_img[3 * p + 2] = a2;
        A.out_depth[p] = Dq[q];
        if constexpr (LAYERS) {
            const float Th = fabsf(TH[q]), Tt = fabsf(TT[q]);
            A.final_T[HW + p] = Th;
            A.out_img[3 * (HW + p) + 0] = fmaf(Th, bg0, H0[q]);
            A.out_img[3 * (HW + p) + 1] = fmaf(Th, bg1, H1[q]);
            A.out_img[3 * (HW + p) + 2] = fmaf(Th, bg2, H2[q]);
            A.final_T[2 * HW + p] = Tt;
            A.out_img[3 * (2 * HW + p) + 0] = fmaf(Tt, bg0, L0[q]);
            A.out_img[3 * (2 * HW + p) + 1] = fmaf(Tt, bg1, L1[q]);
            A.out_img[3 * (2 * HW + p) + 2] = fmaf(Tt, bg2, L2[q]);
        } else {
            // the layer that equals the all-layer here (copy_to: 1 head, 2 tail); the other one is empty: T = 1, C = 0
            const size_t same = (size_t)copy_to * HW + p, blank = (size_t)(3 - copy_to) * HW + p;
            A.final_T[same] = Ta;
            A.out_img[3 * same + 0] = a0; A.out_img[3 * same + 1] = a1; A.out_img[3 * same + 2] = a2;
            A.final_T[blank] = 1.f;
            A.out_img[3 * blank + 0] = fmaf(1.f, bg0, 0.f);
            A.out_img[3 * blank + 1] = fmaf(1.f, bg1, 0.f);
            A.out_img[3 * blank + 2] = fmaf(1.f, bg2, 0.f);
        }
    }
}

template <bool EXACT>
__global__ __launch_bounds__(64) void raster_layers_kernel(const LayerArgs A) {
    __shared__ float4 stage[2][64 * 3];
    __shared__ float stage_d[2][64];
    int t_idx, wv;
    bool is_long;
    if (!packed_launch_map(A.tile_order, A.n_tiles, t_idx, wv, is_long)) return;
    int tile = t_idx;
    if (A.tile_order) tile = A.tile_order[tile];
    if (tile < 0 || tile >= A.n_tiles) return;
    // which layers differ on this tile?  an empty id range, or (own list) no tail entry in the tile: one walk, one copy
    int copy_to = 0;                         // 0: three layers; 1: head == all; 2: tail == all
    if (A.split >= A.n) copy_to = 1;
    else if (A.split <= 0) copy_to = 2;
    else if (A.own_bins != nullptr) {
        const int2 ob = A.own_bins[tile];
        if (ob.y <= ob.x) copy_to = 1;
    }
    if (copy_to == 0) {
        if (is_long) layers_tile<EXACT, 1, 0>(A, tile, wv, stage, stage_d, 0);
        else layers_tile<EXACT, 2, 0>(A, tile, wv, stage, stage_d, 0);
    } else {
        if (is_long) layers_tile<EXACT, 1, 1>(A, tile, wv, stage, stage_d, copy_to);
        else layers_tile<EXACT, 2, 1>(A, tile, wv, stage, stage_d, copy_to);
    }
}

// ------------------------------------------------------------------ the finishing launch
// Everything the reference computes per pixel after the rasterizations (sgn_splatfacto.py:968-996, eval mode), for the
// three layers at once, in the reference's operation order: no fma is formed (this TU is built with -ffp-contract=off),
// so every output equals the eager torch expression bit for bit.
//   rgb            = clamp(clamp(img_all, max=1) * a + sky * (1 - a), 0, 1)         a = 1 - T_all
//   background_rgb = the same from the head layer (its own a)
//   object_rgb     = clamp(clamp(img_tail, max=1), 0, 1)                           (no sky: scene_graph.py:371)
//   depth          = a > 1e-3 ? D / a : 10
//   acc[3]         = 1 - T
// sky == nullptr (use_sky_sphere = False): no blend, rgb = clamp(clamp(img, max=1), 0, 1).
__device__ __forceinline__ float clamp_max1(float v) { return v > 1.f ? 1.f : v; }          // torch.clamp(max=1): NaN stays
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

__global__ __launch_bounds__(256) void layers_finish_kernel(int n_pix, const float *__restrict__ img,
                                                            const float *__restrict__ Ts, const float *__restrict__ D,
                                                            const float *__restrict__ sky, float *__restrict__ rgb,
                                                            float *__restrict__ acc, float *__restrict__ depth) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pix) return;
    const size_t HW = (size_t)n_pix, P = (size_t)p;
    float a[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        a[l] = 1.f - Ts[l * HW + P];
        acc[l * HW + P] = a[l];
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = clamp_max1(img[3 * (l * HW + P) + c]);
            if (sky != nullptr && l < 2) {
                const float front = v * a[l];
                const float back = sky[3 * P + c] * (1.f - a[l]);
                v = front + back;
            }
            rgb[3 * (l * HW + P) + c] = clamp01(v);
        }
    }
    depth[P] = a[0] > 1e-3f ? D[P] / a[0] : 10.f;
}

}  // namespace

SGN_EXPORT int sgn_raster_layers_fwd(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                                     const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                                     const float *conics, const float *colors, const float *opacities,
                                     int opacity_is_logit, const float *background3, const float *depths, int split,
                                     const int32_t *own_ids, const int32_t *own_bins, float *out_img, float *final_Ts,
                                     float *out_depth, void *recs_ws, size_t recs_ws_bytes, int rows_built,
                                     const int32_t *tile_order, const sgn_raster_opts *opts, sgn_stream_t stream) {
    SGN_ARG_CHECK(block_width == 16, -12);                       // the layered walk exists for 16x16 tiles only
    SGN_ARG_CHECK(img_h > 0 && img_w > 0, -1);
    SGN_ARG_CHECK((int64_t)img_h * img_w * 9 < ((int64_t)1 << 31), -1);
    SGN_ARG_CHECK(n_isect >= 0 && n_isect < ((int64_t)1 << 31), -3);
    SGN_ARG_CHECK(tile_bins && background3 && out_img && final_Ts && out_depth, -4);
    SGN_ARG_CHECK(n_isect == 0 || (gaussian_ids_sorted && depths && recs_ws), -5);
    SGN_ARG_CHECK(n >= 0 && recs_ws_bytes >= sgn_raster_workspace_bytes(n, n_isect, opts), -6);
    SGN_ARG_CHECK(split >= 0 && split <= n, -14);
    SGN_ARG_CHECK((own_ids != nullptr) == (own_bins != nullptr), -15);
    sgn_raster_opts o;
    sgn_raster_default_opts(&o);
    if (opts) {
        o.exact_exp = opts->exact_exp ? 1 : 0;
        o.ids_qmask = opts->ids_qmask ? 1 : 0;
        if (opts->batch_fwd > 0) o.batch_fwd = opts->batch_fwd;
    }
    SGN_ARG_CHECK(!o.ids_qmask || n < SGN_QMASK_MAX_IDS, -11);
    if (n_isect > 0 && !rows_built) {
        SGN_ARG_CHECK(xys && conics && colors && opacities, -5);
        const int rc = sgn_raster_build_rows(n, xys, conics, colors, opacities, opacity_is_logit, 0, n, 0, recs_ws,
                                             recs_ws_bytes, nullptr, stream);
        if (rc != 0) return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    LayerArgs A;
    A.W = img_w; A.H = img_h;
    A.tiles_x = (img_w + 15) / 16;
    A.n_tiles = A.tiles_x * ((img_h + 15) / 16);
    A.split = split; A.n = n;
    A.batch_thresh = o.batch_fwd; A.use_qm = o.ids_qmask;
    A.bins = (const int2 *)tile_bins; A.ids = gaussian_ids_sorted;
    A.own_bins = (const int2 *)own_bins; A.own_ids = own_ids;
    A.recs = (const Rec *)recs_ws; A.depths = depths; A.bg = background3; A.tile_order = tile_order;
    A.out_img = out_img; A.final_T = final_Ts; A.out_depth = out_depth;
    const dim3 grid(((A.n_tiles + 7) / 8) * 32 + 32);           // as the packed forward: room for every tile being "long"
    sgn_timing_begin(SGN_T_RASTER_FWD, s);
    if (o.exact_exp) hipLaunchKernelGGL(raster_layers_kernel<true>, grid, dim3(64), 0, s, A);
    else hipLaunchKernelGGL(raster_layers_kernel<false>, grid, dim3(64), 0, s, A);
    sgn_timing_end(SGN_T_RASTER_FWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_layers_finish(int img_h, int img_w, const float *layer_img, const float *layer_Ts,
                                 const float *depth_channel, const float *sky, float *rgb, float *acc, float *depth,
                                 sgn_stream_t stream) {
    SGN_ARG_CHECK(img_h > 0 && img_w > 0 && (int64_t)img_h * img_w * 9 < ((int64_t)1 << 31), -1);
    SGN_ARG_CHECK(layer_img && layer_Ts && depth_channel && rgb && acc && depth, -2);
    const int n_pix = img_h * img_w;
    hipLaunchKernelGGL(layers_finish_kernel, dim3(sgn_cdiv(n_pix, 256)), dim3(256), 0, (hipStream_t)stream, n_pix,
                       layer_img, layer_Ts, depth_channel, sky, rgb, acc, depth);
    SGN_LAUNCH_CHECK();
    return 0;
}
