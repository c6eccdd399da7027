// raster_features.hip — alpha-compositing of K per-Gaussian FEATURE channels over an existing depth list, forward and
// backward, gfx950.  (No upstream counterpart in the 3-channel path; upstream's N-D kernels play this role.)
//
// The 3-channel kernels of raster.hip serve K channels as ceil(K / 3) full passes: every pass walks every tile list
// again and evaluates every sigma / exp / alpha again for three useful fmas per (pixel, Gaussian) pair.  Here a pair's
// alpha is evaluated ONCE per chunk of up to 16 channels: K <= 16 is one walk, K <= 64 is ceil(K / 16) walks inside
// the one call (class logits + depth = 20 channels: two walks where the 3-channel form takes seven, forward and again
// backward).
//
// Arithmetic: the contract in raster.hip's header, operation for operation (this TU is built with -ffp-contract=off
// and spells every fma):
//   sigma = fma(b*dx, dy, fma(hc*dy, dy, (ha*dx)*dx));  alpha = min(0.999, opac * exp(-sigma));
//   skip if sigma < 0 or alpha < 1/255;  nT = T*(1-alpha);  stop (not composited) if nT <= 1e-4;
//   F_c = fma(f_c, alpha*T, F_c);  out_c = fma(T_final, background_c, F_c)
// so every output channel, final_Ts and final_idx are BIT-EQUAL to the same channel of a 3-channel pass over the same
// list (tests/test_gpu_features.py, both exp forms).  The backward follows raster_bwd_tile: ra = rcp(1 - alpha),
// Tn = T ra, fac = alpha Tn, v_alpha = ra (T dotc - bv + c0), v_sigma = -(opac vis) v_alpha (not zeroed by the
// clamp), spatial terms as raw moments, the conic applied once per Gaussian afterwards.  v_alpha is linear in the
// channels, so each chunk walk adds its share of the geometry gradients into the same per-Gaussian sums (the alpha
// image's gradient rides on the first chunk).
//
// Shape: ONE wave64 per 16x16 tile, four pixels per lane (one per 8x8 quadrant), as raster.hip's one-wave form.  The
// tile's ids are read 64 at a time, lane-parallel and one batch ahead; entries whose quadrant bits (ids_qmask lists)
// or bounding box (others) miss the tile's quadrants are never visited.  A visited entry's operands — its 32-byte
// geometry row (x, y, activated opacity, ha | b, hc, ex, ey; built once per call in the workspace) and its CH
// features — are fetched at the wave-uniform id, one entry ahead, and reach the VALU as uniform operands: no LDS, so
// occupancy is set by registers alone.  That traversal is walk_uniform below, upwards for the forward and downwards for
// the backward; the two kernels supply what they do per entry.  Backward: the wave's partial sums (five moments, v_opacity, CH feature
// gradients) are reduced with the transposed permlane-swap + DPP reduction of raster.hip, four values per result
// register, and ONE global_atomic_add_f32 instruction with up to 22 active lanes adds them to the per-Gaussian geometry
// row and straight into v_features.
#include "sgn_common.h"
#include "raster_common.h"

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

constexpr int FEAT_MAX_K = 64;      // channels per call
constexpr int FEAT_MAX_CH = 16;     // channels per walk

// ---- per-Gaussian geometry rows: two float4 per Gaussian (the bbox is build_grec_kernel's, raster.hip)
__global__ __launch_bounds__(256) void feat_rows_kernel(int n, const float *__restrict__ xys,
                                                        const float *__restrict__ conics,
                                                        const float *__restrict__ opac, int opac_is_logit,
                                                        float4 *__restrict__ geo) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const float x = xys[2 * g], y = xys[2 * g + 1];
    const float a = conics[3 * g], b = conics[3 * g + 1], c = conics[3 * g + 2];
    float o = opac[g];
    if (opac_is_logit) o = 1.f / (1.f + expf(-o));
    float ex, ey;
    alpha_box(o, a, b, c, ex, ey);
    geo[2 * (size_t)g + 0] = make_float4(x, y, o, 0.5f * a);
    geo[2 * (size_t)g + 1] = make_float4(b, 0.5f * c, ex, ey);
}

// pixel of (quadrant q, lane) in tile (tx, ty)
__device__ __forceinline__ void quad_pixel(int q, int lane, int tx, int ty, int &i, int &j) {
    j = tx * 16 + (q & 1) * 8 + (lane & 7);
    i = ty * 16 + (q >> 1) * 8 + (lane >> 3);
}

// One visited entry's operands at the wave-uniform id `gid`: the geometry row and the chunk's CH features (channels past
// the chunk's last valid one read the last valid one's address and become 0).
template <int CH>
__device__ __forceinline__ void load_entry(const float4 *__restrict__ geo, const float *__restrict__ feats, int gid, int K,
                                           int c0, int nvalid, float4 &g0, float4 &g1, float (&f)[CH]) {
    g0 = geo[2 * (size_t)gid + 0];
    g1 = geo[2 * (size_t)gid + 1];
    const float *fr = feats + (size_t)gid * (size_t)K + c0;
    if (nvalid == CH) {   // wave-uniform; the usual case: consecutive words, wide scalar loads
#pragma unroll
        for (int c = 0; c < CH; ++c) f[c] = fr[c];
    } else {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float v = fr[min(c, nvalid - 1)];
            f[c] = c < nvalid ? v : 0.f;
        }
    }
}

// this lane's entry of a 64-entry batch: its id (mask bits removed) and the quadrants of the tile it can touch
__device__ __forceinline__ void fetch_id(const int32_t *__restrict__ ids, const float4 *__restrict__ geo, int k, bool in,
                                         int use_qm, int idmask, int tx, int ty, int &gid, unsigned &qrow) {
    gid = 0;
    qrow = 0u;
    if (in) {
        const int raw = ids[k];
        gid = raw & idmask;
        if (use_qm) {
            qrow = (unsigned)raw >> QM_SHIFT;
        } else {
            const float4 g0 = geo[2 * (size_t)gid + 0], g1 = geo[2 * (size_t)gid + 1];
            qrow = row_quadrants(g0.x, g0.y, g1.z, g1.w, tx * 16, ty * 16, true);
        }
    }
}

// The walk of both kernels: `n` positions of the tile's list from `first` on, upwards (DIR = 1) or downwards (DIR = -1).
// The ids (and boxes) of the next 64 positions are in flight while a batch is composited; a visited entry's operands
// are fetched at its wave-uniform id while the entry before it is evaluated.  visit(g0, g1, f, gid, k, qm) gets the
// entry at list position k and the tile's quadrants qm it can touch; false stops the walk.
template <int DIR, int CH, class Visit>
__device__ __forceinline__ void walk_uniform(const int32_t *__restrict__ ids, const float4 *__restrict__ geo,
                                             const float *__restrict__ feats, int K, int c0, int nvalid, int use_qm,
                                             int idmask, int tx, int ty, int first, int n, Visit visit) {
    const int lane = threadIdx.x;
    int gidv, gidv_n = 0;
    unsigned qrow, qrow_n = 0u;
    if (n > 0) fetch_id(ids, geo, first + DIR * lane, lane < n, use_qm, idmask, tx, ty, gidv_n, qrow_n);
    bool go = true;
    for (int b0 = 0; b0 < n && go; b0 += 64) {
        gidv = gidv_n;
        qrow = qrow_n;
        if (b0 + 64 < n)
            fetch_id(ids, geo, first + DIR * (b0 + 64 + lane), b0 + 64 + lane < n, use_qm, idmask, tx, ty, gidv_n, qrow_n);
        unsigned long long todo = __ballot(qrow != 0u);
        if (todo == 0ull) continue;
        int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        unsigned qm = (unsigned)__builtin_amdgcn_readlane((int)qrow, j);
        int gid = __builtin_amdgcn_readlane(gidv, j);
        float4 g0, g1;
        float f[CH];
        load_entry<CH>(geo, feats, gid, K, c0, nvalid, g0, g1, f);
        while (true) {
            const bool more = todo != 0ull;       // wave-uniform
            int jn = j, gidn = gid;
            unsigned qmn = qm;
            float4 n0 = g0, n1 = g1;
            float fn[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) fn[c] = f[c];
            if (more) {                            // the next visited entry's operands, one entry ahead
                jn = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                qmn = (unsigned)__builtin_amdgcn_readlane((int)qrow, jn);
                gidn = __builtin_amdgcn_readlane(gidv, jn);
                load_entry<CH>(geo, feats, gidn, K, c0, nvalid, n0, n1, fn);
            }
            if (!visit(g0, g1, f, gid, first + DIR * (b0 + j), qm)) { go = false; break; }
            if (!more) break;
            j = jn; gid = gidn; qm = qmn; g0 = n0; g1 = n1;
#pragma unroll
            for (int c = 0; c < CH; ++c) f[c] = fn[c];
        }
    }
}

// ------------------------------------------------------------------ forward
template <bool EXACT, int CH>
// (the 16-channel body lands one register over the four-waves-per-SIMD budget on its own: held at 128)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(CH == 16 ? 4 : 1))) void feat_fwd_kernel(
                                                      int W, int H, int tiles_x, int K, int c0,
                                                      const int2 *__restrict__ bins, const int32_t *__restrict__ ids,
                                                      const float4 *__restrict__ geo, const float *__restrict__ feats,
                                                      const float *__restrict__ bg, int use_qm,
                                                      float *__restrict__ out_img, float *__restrict__ final_T,
                                                      int32_t *__restrict__ final_idx) {
    const int lane = threadIdx.x, tile = blockIdx.x;
    const int2 range = bins != nullptr ? bins[tile] : make_int2(0, 0);
    const int idmask = qm_idmask(use_qm);
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int nvalid = min(CH, K - c0);

    // "finished (or outside the image)" is the SIGN of T (raster.hip)
    // (pixel centres are rebuilt per use from quadrant 0's: small integers + 0.5, exact — eight registers less)
    const float pxb = (float)(tx * 16 + (lane & 7)) + 0.5f, pyb = (float)(ty * 16 + (lane >> 3)) + 0.5f;
    float T[4], F[CH][4];
    int last[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int i, j;
        quad_pixel(q, lane, tx, ty, i, j);
        T[q] = (j < W && i < H) ? 1.f : -1.f;
        last[q] = 0;
#pragma unroll
        for (int c = 0; c < CH; ++c) F[c][q] = 0.f;
    }

    // one entry for the tile's pixels; false: every pixel is finished
    auto entry = [&](const float4 &g0, const float4 &g1, const float (&f)[CH], int k, unsigned qm)
                     __attribute__((always_inline)) -> bool {
        unsigned long long live[4], any_live = 0ull;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            live[q] = __ballot(T[q] > 0.f);
            any_live |= live[q];
        }
        if (any_live == 0ull) return false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (live[q] == 0ull || !((qm >> q) & 1u)) continue;   // wave-uniform
            const float dx = g0.x - (pxb + (float)((q & 1) * 8)), dy = g0.y - (pyb + (float)((q >> 1) * 8));
            float s = (g0.w * dx) * dx;
            s = fmaf(g1.y * dy, dy, s);
            const float sigma = fmaf(g1.x * dx, dy, s);
            const float alpha = fminf(0.999f, g0.z * sgn_exp<EXACT>(-sigma));
            const bool valid = T[q] > 0.f && sigma >= 0.f && alpha >= (1.f / 255.f);
            const float nT = T[q] * (1.f - alpha);
            const bool stop = valid && nT <= 1e-4f;
            const bool acc = valid && !stop;
            const float vis = acc ? alpha * T[q] : 0.f;   // lanes that skip or stop add 0: fma(f, 0, F) == F
#pragma unroll
            for (int c = 0; c < CH; ++c) F[c][q] = fmaf(f[c], vis, F[c][q]);
            last[q] = acc ? k : last[q];
            const float Tk = acc ? nT : T[q];
            T[q] = stop ? -Tk : Tk;   // the terminating entry is not composited; T keeps its last value
        }
        return true;
    };

    walk_uniform<1, CH>(ids, geo, feats, K, c0, nvalid, use_qm, idmask, tx, ty, range.x, range.y - range.x,
                        [&](const float4 &g0, const float4 &g1, const float (&f)[CH], int, int k, unsigned qm) {
                            return entry(g0, g1, f, k, qm);
                        });
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int i, j;
        quad_pixel(q, lane, tx, ty, i, j);
        if (!(j < W && i < H)) continue;
        const size_t pix = (size_t)(i * W + j);
        const float Tq = fabsf(T[q]);
        if (c0 == 0) {                 // every chunk walk arrives at the same state; the first one writes it
            final_T[pix] = Tq;
            final_idx[pix] = last[q];
        }
        float *o = out_img + pix * (size_t)K + c0;
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (c < nvalid) o[c] = fmaf(Tq, bg != nullptr ? bg[c0 + c] : 0.f, F[c][q]);
    }
}

// ------------------------------------------------------------------ backward
// (the wave's partial sums go through raster_common.h's transposed reduction: reduce4(a, b, c, d) leaves the wave totals
// of a, c, b, d in rows 0, 1, 2, 3)
constexpr int GW_FLOATS = 8;   // per-Gaussian geometry sums: m_x m_y s_xx s_xy | s_yy v_opacity 0 0

template <bool EXACT, int CH>
__global__ __launch_bounds__(64) void feat_bwd_kernel(int W, int H, int tiles_x, int K, int c0,
                                                      const int2 *__restrict__ bins, const int32_t *__restrict__ ids,
                                                      const float4 *__restrict__ geo, const float *__restrict__ feats,
                                                      const float *__restrict__ bg, int use_qm,
                                                      const float *__restrict__ final_T,
                                                      const int32_t *__restrict__ final_idx,
                                                      const float *__restrict__ v_out,
                                                      const float *__restrict__ v_out_alpha, float alpha_clamp,
                                                      float *__restrict__ gws, float *__restrict__ v_feats) {
    const int lane = threadIdx.x, tile = blockIdx.x;
    const int2 range = bins[tile];
    if (range.x >= range.y) return;
    const int idmask = qm_idmask(use_qm);
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int nvalid = min(CH, K - c0);

    // per-pixel state; algebra as raster_bwd_tile: v_alpha = ra (T_before dotc - bv + c0v),
    // c0v = T_final (v_out_alpha - sum_c bg_c v_out_c), bv += fac dotc
    const float pxb = (float)(tx * 16 + (lane & 7)) + 0.5f, pyb = (float)(ty * 16 + (lane >> 3)) + 0.5f;
    float T[4], c0v[4], bv[4], vo[CH][4];
    int kfin[4], pixi[4];
    int kmax_l = -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int i, j;
        quad_pixel(q, lane, tx, ty, i, j);
        const bool inside = j < W && i < H;
        pixi[q] = inside ? i * W + j : -1;
        kfin[q] = inside ? final_idx[pixi[q]] : -1;   // -1: this slot never participates
        kmax_l = max(kmax_l, kfin[q]);
    }
    int kmax = __builtin_amdgcn_readfirstlane(wave_max_i(kmax_l));
    kmax = min(kmax, range.y - 1);
    if (kmax < range.x) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool inside = pixi[q] >= 0;
        const size_t pix = inside ? (size_t)pixi[q] : 0;
        const float Tf = inside ? final_T[pix] : 1.f;
        T[q] = Tf;
        // a pixel nothing was composited onto (T stayed exactly 1) takes no part: its incoming gradients are not read
        // (raster_bwd_tile: they may hold 0 / 0 of a `where`)
        const bool live = inside && Tf < 1.f;
        float sb = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            vo[c][q] = (live && v_out != nullptr && c < nvalid) ? v_out[pix * (size_t)K + c0 + c] : 0.f;
            sb = fmaf((bg != nullptr && c < nvalid) ? bg[c0 + c] : 0.f, vo[c][q], sb);
        }
        // the alpha image's gradient rides on the first chunk's walk
        const float voa = (live && c0 == 0 && v_out_alpha != nullptr) ? v_out_alpha[pix] : 0.f;
        c0v[q] = Tf * (voa - sb);
        bv[q] = 0.f;
    }

    // one entry of the reverse walk
    auto entry = [&](const float4 &g0, const float4 &g1, const float (&f)[CH], int gid, int k, unsigned qm)
                     __attribute__((always_inline)) {
        float m_x = 0.f, m_y = 0.f, s_xx = 0.f, s_xy = 0.f, s_yy = 0.f, g_o = 0.f;
        float g_f[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) g_f[c] = 0.f;
        bool any = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!((qm >> q) & 1u) || __ballot(k <= kfin[q]) == 0ull) continue;   // wave-uniform
            const float dx = g0.x - (pxb + (float)((q & 1) * 8)), dy = g0.y - (pyb + (float)((q >> 1) * 8));
            const float t1 = g0.w * dx, t2 = g1.y * dy, t3 = g1.x * dx;
            const float sigma = fmaf(t3, dy, fmaf(t2, dy, t1 * dx));
            const float vis = sgn_exp<EXACT>(-sigma);
            const float av = g0.z * vis;
            const float alpha = fminf(alpha_clamp, av);
            const bool valid = (k <= kfin[q]) && sigma >= 0.f && alpha >= (1.f / 255.f);
            const float ra = __builtin_amdgcn_rcpf(1.f - alpha);
            const float Tn = T[q] * ra;
            const float fac = alpha * Tn;
            float dotc = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) dotc = fmaf(f[c], vo[c][q], dotc);
            const float v_alpha = ra * fmaf(T[q], dotc, c0v[q] - bv[q]);
            const float vm = valid ? v_alpha : 0.f;
            const float facm = valid ? fac : 0.f;
            bv[q] = fmaf(facm, dotc, bv[q]);
            T[q] = valid ? Tn : T[q];
            const float vs = -av * vm;                  // v_sigma (upstream: not zeroed by the clamp)
            const float p = vs * dx, qq = vs * dy;
            m_x += p;
            m_y += qq;
            s_xx = fmaf(p, dx, s_xx);
            s_xy = fmaf(p, dy, s_xy);
            s_yy = fmaf(qq, dy, s_yy);
#pragma unroll
            for (int c = 0; c < CH; ++c) g_f[c] = fmaf(facm, vo[c][q], g_f[c]);
            g_o = fmaf(vis, vm, g_o);
            any = any || valid;
        }
        if (__ballot(any) == 0ull) return;   // wave-uniform
        // value index v: 0..5 the geometry sums, 6, 7 unused, 8 + c feature channel c.  Register i of the reduction holds
        // value 4 i + rowmap(row) in every lane of a 16-lane row; lane (row, i) adds it.
        constexpr int NR = (8 + CH + 3) / 4;
        float u[NR];
        u[0] = reduce4(m_x, m_y, s_xx, s_xy);
        u[1] = reduce4(s_yy, g_o, 0.f, 0.f);
        float gp[4 * (NR - 2)];
#pragma unroll
        for (int c = 0; c < 4 * (NR - 2); ++c) gp[c] = c < CH ? g_f[c < CH ? c : 0] : 0.f;
#pragma unroll
        for (int i = 2; i < NR; ++i) u[i] = reduce4(gp[4 * i - 8], gp[4 * i - 7], gp[4 * i - 6], gp[4 * i - 5]);
        const int col = lane & 15, row = lane >> 4;
        const int v = 4 * col + (((row & 1) << 1) | (row >> 1));   // rows 0, 1, 2, 3 hold values 0, 2, 1, 3 of a register
        float mine = u[0];
#pragma unroll
        for (int i = 1; i < NR; ++i) mine = (col == i) ? u[i] : mine;
        if (col < NR) {
            if (v < 6) unsafeAtomicAdd(gws + (size_t)gid * GW_FLOATS + v, mine);
            else if (v >= 8 && v - 8 < nvalid) unsafeAtomicAdd(v_feats + (size_t)gid * (size_t)K + c0 + (v - 8), mine);
        }
    };

    walk_uniform<-1, CH>(ids, geo, feats, K, c0, nvalid, use_qm, idmask, tx, ty, kmax, kmax - range.x + 1,
                         [&](const float4 &g0, const float4 &g1, const float (&f)[CH], int gid, int k, unsigned qm) {
                             entry(g0, g1, f, gid, k, qm);
                             return true;
                         });
}

// per-Gaussian geometry sums -> v_xy, v_conic, v_opacity (unpack_grads_kernel of raster.hip without the colours)
__global__ __launch_bounds__(256) void feat_unpack_kernel(int n, const float *__restrict__ gws,
                                                          const float *__restrict__ conics,
                                                          const float *__restrict__ opac, int opac_is_logit,
                                                          float *__restrict__ v_xy, float *__restrict__ v_conic,
                                                          float *__restrict__ v_opac) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 a = reinterpret_cast<const float4 *>(gws)[2 * (size_t)i + 0];
    const float4 b = reinterpret_cast<const float4 *>(gws)[2 * (size_t)i + 1];
    moments_to_grads(conics + 3 * (size_t)i, a, b.x, v_xy + 2 * (size_t)i, v_conic + 3 * (size_t)i);
    float vo = b.y;
    if (opac_is_logit) {              // opac holds logits: chain through the fused sigmoid
        const float sg = 1.f / (1.f + expf(-opac[i]));
        vo = vo * sg * (1.f - sg);
    }
    v_opac[i] = vo;
}

// width of the chunk walk that starts at channel c0 of K
int chunk_width(int K, int c0) {
    const int r = K - c0;
    if (r >= FEAT_MAX_CH) return FEAT_MAX_CH;
    int w = 1;
    while (w < r) w <<= 1;
    return w;
}

int check_common(const char *fn, int img_h, int img_w, int block_width, int n, int n_channels, int64_t n_isect) {
    if (block_width != 16) {
        sgn_set_error("%s: argument check failed: block_width == 16", fn);
        return -12;
    }
    if (!(img_h > 0 && img_w > 0 && n >= 0)) {
        sgn_set_error("%s: argument check failed: img_h > 0 && img_w > 0 && n >= 0", fn);
        return -1;
    }
    if (!(n_channels >= 1 && n_channels <= FEAT_MAX_K)) {
        sgn_set_error("%s: argument check failed: 1 <= n_channels <= 64", fn);
        return -13;
    }
    if (!((int64_t)img_h * img_w < ((int64_t)1 << 31))) {
        sgn_set_error("%s: argument check failed: img_h * img_w < 2^31", fn);
        return -1;
    }
    if (!(n_isect >= 0 && n_isect < ((int64_t)1 << 31))) {
        sgn_set_error("%s: argument check failed: 0 <= n_isect < 2^31", fn);
        return -3;
    }
    return 0;
}

}  // namespace

SGN_EXPORT size_t sgn_raster_features_workspace_bytes(int n) {
    // geometry rows (32 B) + the backward's per-Gaussian geometry sums (32 B)
    return (size_t)(n > 0 ? n : 1) * (size_t)(8 + GW_FLOATS) * sizeof(float);
}

#define SGN_FEAT_DISPATCH(KERNEL, EX, CH, ...)                                                                   \
    do {                                                                                                         \
        switch (CH) {                                                                                            \
        case 1: hipLaunchKernelGGL((KERNEL<EX, 1>), grid, dim3(64), 0, s, __VA_ARGS__); break;                   \
        case 2: hipLaunchKernelGGL((KERNEL<EX, 2>), grid, dim3(64), 0, s, __VA_ARGS__); break;                   \
        case 4: hipLaunchKernelGGL((KERNEL<EX, 4>), grid, dim3(64), 0, s, __VA_ARGS__); break;                   \
        case 8: hipLaunchKernelGGL((KERNEL<EX, 8>), grid, dim3(64), 0, s, __VA_ARGS__); break;                   \
        default: hipLaunchKernelGGL((KERNEL<EX, 16>), grid, dim3(64), 0, s, __VA_ARGS__); break;                 \
        }                                                                                                        \
    } while (0)

SGN_EXPORT int sgn_raster_features_fwd(int img_h, int img_w, int block_width, int n, int n_channels, int64_t n_isect,
                                       const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                                       const float *conics, const float *features, const float *opacities,
                                       int opacity_is_logit, const float *background, float *out_img, float *final_Ts,
                                       int32_t *final_idx, void *ws, size_t ws_bytes, const sgn_raster_opts *opts,
                                       sgn_stream_t stream) {
    const int rc = check_common(__func__, img_h, img_w, block_width, n, n_channels, n_isect);
    if (rc != 0) return rc;
    SGN_ARG_CHECK(out_img && final_Ts && final_idx, -4);
    SGN_ARG_CHECK(n_isect == 0 || (gaussian_ids_sorted && tile_bins && xys && conics && features && opacities && ws), -5);
    SGN_ARG_CHECK(n_isect == 0 || n > 0, -5);
    SGN_ARG_CHECK(n_isect == 0 || ws_bytes >= sgn_raster_features_workspace_bytes(n), -6);
    const int use_qm = (opts && opts->ids_qmask) ? 1 : 0, exact = (opts && opts->exact_exp) ? 1 : 0;
    SGN_ARG_CHECK(!use_qm || n < SGN_QMASK_MAX_IDS, -11);
    hipStream_t s = (hipStream_t)stream;
    const int tiles_x = (img_w + 15) / 16, n_tiles = tiles_x * ((img_h + 15) / 16);
    const int K = n_channels;
    const float4 *geo = (const float4 *)ws;
    if (n_isect > 0)
        hipLaunchKernelGGL(feat_rows_kernel, dim3(sgn_cdiv(n, 256)), dim3(256), 0, s, n, xys, conics, opacities,
                           opacity_is_logit ? 1 : 0, (float4 *)ws);
    // n_isect == 0: every list is empty (the bins are not read): background, T = 1, idx = 0
    const int2 *bins = n_isect > 0 ? (const int2 *)tile_bins : nullptr;
    const dim3 grid(n_tiles);
    sgn_timing_begin(SGN_T_RASTER_FWD, s);
    for (int c0 = 0; c0 < K; c0 += FEAT_MAX_CH) {
        const int ch = chunk_width(K, c0);
        if (exact)
            SGN_FEAT_DISPATCH(feat_fwd_kernel, true, ch, img_w, img_h, tiles_x, K, c0, bins, gaussian_ids_sorted, geo,
                              features, background, use_qm, out_img, final_Ts, final_idx);
        else
            SGN_FEAT_DISPATCH(feat_fwd_kernel, false, ch, img_w, img_h, tiles_x, K, c0, bins, gaussian_ids_sorted, geo,
                              features, background, use_qm, out_img, final_Ts, final_idx);
    }
    sgn_timing_end(SGN_T_RASTER_FWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_raster_features_bwd(int img_h, int img_w, int block_width, int n, int n_channels, int64_t n_isect,
                                       const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const float *xys,
                                       const float *conics, const float *features, const float *opacities,
                                       int opacity_is_logit, const float *background, const float *final_Ts,
                                       const int32_t *final_idx, const float *v_out_img, const float *v_out_alpha,
                                       float alpha_clamp_bwd, float *v_xy, float *v_conic, float *v_features,
                                       float *v_opacity, void *ws, size_t ws_bytes, const sgn_raster_opts *opts,
                                       sgn_stream_t stream) {
    const int rc = check_common(__func__, img_h, img_w, block_width, n, n_channels, n_isect);
    if (rc != 0) return rc;
    if (n == 0) return 0;
    SGN_ARG_CHECK(v_xy && v_conic && v_features && v_opacity && conics && opacities && ws, -4);
    SGN_ARG_CHECK(n_isect == 0 || (gaussian_ids_sorted && tile_bins && xys && features && final_Ts && final_idx), -5);
    SGN_ARG_CHECK(ws_bytes >= sgn_raster_features_workspace_bytes(n), -6);
    SGN_ARG_CHECK(alpha_clamp_bwd > 0.f && alpha_clamp_bwd < 1.f, -7);
    const int use_qm = (opts && opts->ids_qmask) ? 1 : 0, exact = (opts && opts->exact_exp) ? 1 : 0;
    SGN_ARG_CHECK(!use_qm || n < SGN_QMASK_MAX_IDS, -11);
    hipStream_t s = (hipStream_t)stream;
    const int tiles_x = (img_w + 15) / 16, n_tiles = tiles_x * ((img_h + 15) / 16);
    const int K = n_channels;
    float4 *geo = (float4 *)ws;
    float *gws = (float *)ws + (size_t)n * 8;
    SGN_HIP_CHECK(hipMemsetAsync(gws, 0, (size_t)n * GW_FLOATS * sizeof(float), s));
    SGN_HIP_CHECK(hipMemsetAsync(v_features, 0, (size_t)n * (size_t)K * sizeof(float), s));
    if (n_isect > 0) {
        hipLaunchKernelGGL(feat_rows_kernel, dim3(sgn_cdiv(n, 256)), dim3(256), 0, s, n, xys, conics, opacities,
                           opacity_is_logit ? 1 : 0, geo);
        const dim3 grid(n_tiles);
        sgn_timing_begin(SGN_T_RASTER_BWD, s);
        for (int c0 = 0; c0 < K; c0 += FEAT_MAX_CH) {
            const int ch = chunk_width(K, c0);
            if (exact)
                SGN_FEAT_DISPATCH(feat_bwd_kernel, true, ch, img_w, img_h, tiles_x, K, c0, (const int2 *)tile_bins,
                                  gaussian_ids_sorted, (const float4 *)geo, features, background, use_qm, final_Ts,
                                  final_idx, v_out_img, v_out_alpha, alpha_clamp_bwd, gws, v_features);
            else
                SGN_FEAT_DISPATCH(feat_bwd_kernel, false, ch, img_w, img_h, tiles_x, K, c0, (const int2 *)tile_bins,
                                  gaussian_ids_sorted, (const float4 *)geo, features, background, use_qm, final_Ts,
                                  final_idx, v_out_img, v_out_alpha, alpha_clamp_bwd, gws, v_features);
        }
        sgn_timing_end(SGN_T_RASTER_BWD, s);
    }
    hipLaunchKernelGGL(feat_unpack_kernel, dim3(sgn_cdiv(n, 256)), dim3(256), 0, s, n, (const float *)gws, conics,
                       opacities, opacity_is_logit ? 1 : 0, v_xy, v_conic, v_opacity);
    SGN_LAUNCH_CHECK();
    return 0;
}
