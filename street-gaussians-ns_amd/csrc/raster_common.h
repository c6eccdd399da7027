// What the raster translation units (raster.hip, raster_absgrad.hip, raster_layers.hip, raster_features.hip) share: the
// 48-byte row, the two exp forms, the quadrant tests, the wave helpers (maximum, the transposed permlane-swap reduction),
// the per-Gaussian arithmetic around the walks (the alpha >= 1/255 box, moments -> gradients), the block -> (tile, wave)
// map of the packed launch, the two ways through a depth list — walk_chase and walk_staged — and the backward body,
// raster_bwd_tile, which raster.hip instantiates plain and raster_absgrad.hip with the absgrad statistic.  A kernel
// supplies what it does per entry (and per batch); the traversal, with its prefetch discipline, is written here once.
// At the end, the host side of the reverse walks: one kernel pointer type, a table of launch shapes per family, and the
// one launcher and the one check-and-prepare step (both in raster.hip) every backward entry goes through.
// The arithmetic contract is in raster.hip's header; all units are built with -ffp-contract=off -fno-slp-vectorize, so
// shared source gives the same bits in each.
#pragma once
#include "sgn_common.h"

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

struct __attribute__((aligned(16))) Rec {
    float x, y, opac, ha;   // ha = 0.5 * conic.x
    float b, hc, r, g;      // b = conic.y, hc = 0.5 * conic.z
    float bl;               // blue
    int gid;                // Gaussian id (backward scatter target)
    float ex, ey;           // half-extents of the bbox of {alpha >= 1/255} (+margin); < 0: never visible
};
static_assert(sizeof(Rec) == SGN_RECORD_FLOATS * sizeof(float), "record size");

__device__ __forceinline__ float exp_portable(float x) {
    // same recipe as oracle/c/sgn_oracle.c exp_portable (written independently; bit-identical)
    float t = x * 1.44269504088896341f;
    t = fminf(fmaxf(t, -125.0f), 126.0f);
    const float n = __builtin_rintf(t);
    const float f = t - n;
    float p = 1.53533063e-4f;
    p = fmaf(p, f, 1.33988744e-3f);
    p = fmaf(p, f, 9.61843736e-3f);
    p = fmaf(p, f, 5.55035681e-2f);
    p = fmaf(p, f, 2.40226488e-1f);
    p = fmaf(p, f, 6.93147182e-1f);
    p = fmaf(p, f, 1.0f);
    return ldexpf(p, (int)n);
}

template <bool EXACT>
__device__ __forceinline__ float sgn_exp(float x) {
    if constexpr (EXACT) return exp_portable(x);
    else return __expf(x);
}

// Which of the tile's four 8x8 quadrants can this Gaussian touch?  Lanes 0..3 each test one quadrant
// (|centre distance| <= half-extent + 3.5 px, the half-span of the quadrant's pixel centres), the ballot
// turns the answers into a wave-uniform 4-bit mask that the per-quadrant branches test in the scalar unit.
__device__ __forceinline__ unsigned quadrant_mask(const Rec &g, float qcx, float qcy, bool enable) {
    if (!enable) return 0xFu;
    const bool hit = fabsf(g.x - qcx) <= g.ex + 3.5f && fabsf(g.y - qcy) <= g.ey + 3.5f;
    return (unsigned)(__ballot(hit) & 0xFull);
}

// Quadrant masks handed in with the list (sgn_raster_opts.ids_qmask, include/sgn_rast.h: sgn_bin_intersect with
// quadrant_masks): bits 28-31 of an id word say which quadrants the entry can touch — the exact convex test, done once
// by the emission — and the kernels neither run the box test above per entry nor evaluate the ~10 % of quadrants the
// box lets through although the ellipse misses them.  A row build_grec_kernel made inert (window passes: ex < 0) keeps
// answering "none".
constexpr int QM_SHIFT = SGN_QMASK_ID_BITS;
__device__ __forceinline__ int qm_idmask(int use_qm) { return use_qm ? (SGN_QMASK_MAX_IDS - 1) : -1; }
__device__ __forceinline__ unsigned qm_bits(int raw_id, float ex) {
    return __float_as_int(ex) < 0 ? 0u : ((unsigned)raw_id >> QM_SHIFT);
}

// Batched path: every lane holds ONE row of the batch and tests all four quadrants for it (lane-parallel over
// 64 entries instead of once per entry), so entries that cannot touch this wave's pixels are never visited.
__device__ __forceinline__ unsigned row_quadrants(float gx, float gy, float ex, float ey, int tile_x0, int tile_y0,
                                                  bool enable) {
    if (!enable) return 0xFu;
    unsigned m = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float cx = (float)(tile_x0 + (q & 1) * 8) + 4.0f, cy = (float)(tile_y0 + (q >> 1) * 8) + 4.0f;
        if (fabsf(gx - cx) <= ex + 3.5f && fabsf(gy - cy) <= ey + 3.5f) m |= 1u << q;
    }
    return m;
}

// ---- wave helpers ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// Transposed wave reduction.  gfx950's v_permlane32_swap / v_permlane16_swap exchange half-waves / odd-even rows BETWEEN
// two registers, so one swap + one add folds two values at once; four DPP adds finish each 16-lane row.
template <int CTRL>
__device__ __forceinline__ float dpp_get(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row_sum_dpp(float v) {   // every lane ends with its 16-lane row total
    v += dpp_get<0xB1>(v);    // quad_perm:[1,0,3,2]
    v += dpp_get<0x4E>(v);    // quad_perm:[2,3,0,1]
    v += dpp_get<0x141>(v);   // row_half_mirror
    v += dpp_get<0x140>(v);   // row_mirror
    return v;
}
__device__ __forceinline__ float fold32(float a, float b) {   // lanes 0-31: a[l]+a[l+32]; lanes 32-63: same of b
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float fold16(float a, float b) {   // rows: [a.r0+a.r1, b.r0+b.r1, a.r2+a.r3, b.r2+b.r3]
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// rows 0, 1, 2, 3 of the result hold the wave totals of a, c, b, d
__device__ __forceinline__ float reduce4(float a, float b, float c, float d) {
    return row_sum_dpp(fold16(fold32(a, b), fold32(c, d)));
}

// ---- per-Gaussian arithmetic around the walks -----------------------------------------------------------------------
// Half-extents of the bbox of the region where alpha = o*exp(-sigma) can reach 1/255: sigma <= s = ln(255 o) (+1 %
// margin); x half-extent sqrt(2 s c / D), y half-extent sqrt(2 s a / D), D = ac - b^2.  The raster kernels skip the 8x8
// quadrants it misses (no valid pixel there => results unchanged).  < 0: never visible.
__device__ __forceinline__ void alpha_box(float o, float a, float b, float c, float &ex, float &ey) {
    const float s = (o * 255.f > 0.f) ? logf(255.f * o) + 0.01f : -1.f;
    const float D = a * c - b * b;
    ex = -1.f; ey = -1.f;
    if (s >= 0.f) {
        const bool proper = a > 0.f && c > 0.f && D > 0.f;
        ex = proper ? sqrtf(2.f * s * c / D) + 1e-3f : 3.0e38f;
        ey = proper ? sqrtf(2.f * s * a / D) + 1e-3f : 3.0e38f;
    }
}

// Raw moments (m_x, m_y, s_xx, s_xy | s_yy) of a Gaussian's v_sigma -> gradients with its conic (A, B, C) at conic:
// sigma = (A dx^2 + C dy^2) / 2 + B dx dy, so v_xy = (A m_x + B m_y, B m_x + C m_y), v_conic = (s_xx / 2, s_xy, s_yy / 2)
// ([1] is the TRUE dL/dB).
__device__ __forceinline__ void moments_to_grads(const float *__restrict__ conic, const float4 &m, float s_yy,
                                                 float *__restrict__ v_xy, float *__restrict__ v_conic) {
    const float A = conic[0], B = conic[1], C = conic[2];
    v_xy[0] = fmaf(A, m.x, B * m.y);
    v_xy[1] = fmaf(B, m.x, C * m.y);
    v_conic[0] = 0.5f * m.z; v_conic[1] = m.w; v_conic[2] = 0.5f * s_yy;
}

// ---- the packed launch: block -> (position in the launch order, wave) -----------------------------------------------
// The first n_long tiles of the launch order (sgn_tile_order with long_thresh: the longest lists) get four waves each,
// the others two.  Blocks come in groups of eight tiles (8 x 4, then 8 x 2 blocks): block b runs on XCD b % 8, so a
// tile's waves share an XCD (and its L2) and are dispatched together, longest tiles first.  No block inside the two
// regions is empty: interleaving waves that exit at once with working ones left half of the SIMDs idle (the dispatcher
// places consecutive workgroups round-robin), 267 vs 159 us on the benchmark scene.  false: this block has no tile.
__device__ __forceinline__ bool packed_launch_map(const int32_t *__restrict__ tile_order, int n_tiles, int &t_idx,
                                                  int &wv, bool &is_long) {
    const int n_long = tile_order ? min(max(tile_order[n_tiles], 0), n_tiles) : 0;
    const int b_long = ((n_long + 7) >> 3) << 5;
    const int b = (int)blockIdx.x;
    is_long = b < b_long;
    if (is_long) {
        t_idx = (b >> 5) * 8 + (b & 7);
        wv = (b >> 3) & 3;
        return t_idx < n_long;
    }
    const int b2 = b - b_long;
    t_idx = n_long + (b2 >> 4) * 8 + (b2 & 7);
    wv = (b2 >> 3) & 1;
    return t_idx < n_tiles;
}

// ---- the two ways through a depth list ------------------------------------------------------------------------------
// Both visit positions of `ids` from `first` on, upwards (DIR = 1, the forward) or downwards (DIR = -1, the backward's
// reverse walk) — walk_chase to `last` inclusive, walk_staged `n` of them — and stop when the visitor returns false.  DEPTH: depths[id] rides along (0 otherwise).
//
// walk_chase: ids[k] -> row with two dependent scalar loads, the id two entries ahead and the row one entry ahead, so the
// operands arrive in SGPRs and only the entries actually walked are ever fetched.  visit(row, raw id word, k, depth).
template <int DIR, bool DEPTH, class Visit>
__device__ __forceinline__ void walk_chase(const int32_t *__restrict__ ids, const Rec *__restrict__ recs,
                                           const float *__restrict__ depths, int idmask, int first, int last, Visit visit) {
    if (DIR > 0 ? first > last : first < last) return;
    int idc = ids[first];              // raw id word (mask bits included)
    Rec cur = recs[idc & idmask];
    float dcur = 0.f;
    if constexpr (DEPTH) dcur = depths[idc & idmask];
    int idn = ids[DIR > 0 ? min(first + 1, last) : max(first - 1, last)];
    for (int k = first; DIR > 0 ? k <= last : k >= last; k += DIR) {
        const Rec nxt = recs[idn & idmask];   // scalar prefetch of the next row
        float dnxt = 0.f;
        if constexpr (DEPTH) dnxt = depths[idn & idmask];
        const int idnn = idn;
        idn = ids[DIR > 0 ? min(k + 2, last) : max(k - 2, last)];
        if (!visit(cur, idc, k, dcur)) return;
        cur = nxt;
        dcur = dnxt;
        idc = idnn;
    }
}

// entry j of a staged batch
__device__ __forceinline__ Rec staged_rec(const float4 *sb, int j) {
    Rec cur;
    const float4 a0 = sb[j * 3 + 0], a1 = sb[j * 3 + 1], a2 = sb[j * 3 + 2];
    cur.x = a0.x; cur.y = a0.y; cur.opac = a0.z; cur.ha = a0.w;
    cur.b = a1.x; cur.hc = a1.y; cur.r = a1.z; cur.g = a1.w;
    cur.bl = a2.x; cur.gid = __float_as_int(a2.y); cur.ex = a2.z; cur.ey = a2.w;
    return cur;
}

// walk_staged: the one-entry scalar look-ahead leaves a lone wave latency-bound on a long list (a dependent id -> row
// load pair per entry), so 64-entry batches go through wave-private LDS instead: lane l gathers the row of position
// first + DIR (64 bi + l) with vector loads a whole batch ahead, and the entries are read back with broadcast
// ds_read_b128.  No barrier: the workgroup is this one wave and its LDS ops retire in order.  The prefetched registers
// are first used AFTER the batch is composited, and what the batch needs of them (the rows' quadrant masks, the raw id
// words) is snapshot before the prefetch overwrites it.
//   row_mask(raw id word, r0, r2)   this lane's row: which of the wave's quadrants it can touch (0: never visited)
//   batch(in_batch, raw id word)    once per batch, before its entries: this lane's row of it (in_batch: it has one)
//   visit(row, j, k, mask, depth)   entry j of the batch = list position k; mask = its row_mask
template <int DIR, bool DEPTH, class RowMask, class Batch, class Visit>
__device__ __forceinline__ void walk_staged(const int32_t *__restrict__ ids, const Rec *__restrict__ recs,
                                            const float *__restrict__ depths, int idmask, int first, int n,
                                            float4 (*stage)[64 * 3], float (*stage_d)[64], RowMask row_mask,
                                            Batch batch, Visit visit) {
    const int lane = threadIdx.x;
    const int nb = (n + 63) >> 6;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
    float rd = 0.f;      // DEPTH: the depth of this lane's row of the batch in flight
    int rid = 0;         // raw id word of this lane's row (quadrant bits on top)
    auto fetch = [&](int bi) __attribute__((always_inline)) {
        const int o = (bi << 6) + lane;
        if (o < n) {
            rid = ids[first + DIR * o];
            const int id = rid & idmask;
            const float4 *p = reinterpret_cast<const float4 *>(recs + id);
            r0 = p[0]; r1 = p[1]; r2 = p[2];
            if constexpr (DEPTH) rd = depths[id];
        }
    };
    fetch(0);
    stage[0][lane * 3 + 0] = r0; stage[0][lane * 3 + 1] = r1; stage[0][lane * 3 + 2] = r2;
    if constexpr (DEPTH) stage_d[0][lane] = rd;
    unsigned qrow = row_mask(rid, r0, r2);
    int rrow = rid;
    bool go = true;
    for (int bi = 0; bi < nb && go; ++bi) {
        const int cnt = min(64, n - (bi << 6));
        unsigned long long todo = __ballot(lane < cnt && qrow != 0u);  // entries that can touch my pixels
        batch(lane < cnt, rrow);
        const unsigned qcur = qrow;
        if (bi + 1 < nb) fetch(bi + 1);   // next batch: in flight while this one is composited
        const float4 *sb = stage[bi & 1];
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            float dep = 0.f;
            if constexpr (DEPTH) dep = stage_d[bi & 1][j];
            if (!visit(staged_rec(sb, j), j, first + DIR * ((bi << 6) + j), (unsigned)__builtin_amdgcn_readlane((int)qcur, j),
                       dep)) {
                go = false;
                break;
            }
        }
        if (go && bi + 1 < nb) {          // first use of the prefetched registers
            float4 *sn = stage[(bi + 1) & 1];
            sn[lane * 3 + 0] = r0; sn[lane * 3 + 1] = r1; sn[lane * 3 + 2] = r2;
            if constexpr (DEPTH) stage_d[(bi + 1) & 1][lane] = rd;
            qrow = row_mask(rid, r0, r2);
            rrow = rid;
        }
    }
}

// ---- the backward body ----------------------------------------------------------------------------------------------
// pixel of (slot q, lane) inside tile (tx,ty).  block 16: four 8x8 quadrants; otherwise linear.
__device__ __forceinline__ void slot_pixel(int q, int lane, int B, int &ox, int &oy, bool &in_tile) {
    if (B == 16) {
        ox = (q & 1) * 8 + (lane & 7);
        oy = (q >> 1) * 8 + (lane >> 3);
        in_tile = true;
    } else {
        const int p = q * 64 + lane;
        ox = p % B;
        oy = p / B;
        in_tile = p < B * B;
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The nine per-Gaussian partial gradients (REDUCE == 1) go through the transposed reduction above: after the
// 32- and 16-lane folds three registers hold, per 16-lane row, t0 = [v0 v2 v1 v3], t1 = [v4 v6 v5 v7], t2 = [v8 0 0 0];
// four DPP adds finish each row.  28 cross-lane ops instead of 54 shuffles.

// grad_ws row layout (12 floats / Gaussian): 0,1 m_x, m_y | 2,3,4 s_xx, s_xy, s_yy (raw moments; the conic is applied by
// unpack_grads_kernel) | 5,6,7 v_rgb | 8 v_opacity | 9,10 absgrad (ABSGRAD only; zero otherwise) | 11 unused
//
// ABSGRAD (raster_absgrad.hip; off in every instantiation of raster.hip, whose arithmetic and order it leaves alone):
// the absgrad statistic of AbsGS, sum over the pixels of |dL/d xy| of this Gaussian.  The per-pixel gradient is the conic
// applied to the pixel's (p, q) = vs * (dx, dy) — what the moments sum BEFORE the conic — so it has to be formed here,
// per evaluated (pixel, entry) pair.  Contract (every fma spelled, -ffp-contract=off):
//   A = ha + ha,  C = hc + hc                         once per entry (exact: the row stores the halves)
//   ax += fabsf(fmaf(A, p, b * q))
//   ay += fabsf(fmaf(b, p, C * q))
// An invalid lane contributes 0 without a select of its own: vs = -av * vm with vm = 0 there, so p = q = +-0.  ax, ay are
// reduced with the nine sums — lanes 9, 10 of the butterfly form; rows 2, 1 of t2 = [v8 ay ax 0] in the swap form, one
// more swap — and added into slots 9, 10 of the Gaussian's workspace row.
template <bool EXACT, int REDUCE, int QPW, bool ADAPT, bool ABSGRAD = false>
__device__ __forceinline__ void raster_bwd_tile(int tile, int wv, int W, int H, int B, int tiles_x,
                                                const int2 *__restrict__ bins, const Rec *__restrict__ recs,
                                                const int32_t *__restrict__ ids, const float *__restrict__ bg,
                                                const float *__restrict__ final_T,
                                                const int32_t *__restrict__ final_idx,
                                                const float *__restrict__ v_out,
                                                const float *__restrict__ v_out_alpha, float alpha_clamp,
                                                float *__restrict__ grad_ws, int dbg, int adapt_thresh,
                                                int batch_thresh, int use_qm) {
    static_assert(!ADAPT || QPW == 4, "adaptive splitting starts from the 4-quadrant wave");
    const bool qm_on = use_qm != 0 && B == 16;      // wave-uniform
    const int idmask = qm_idmask(use_qm);
    const int q0 = ADAPT ? 0 : wv * QPW;
    const int lane = threadIdx.x;
    const int2 range = bins[tile];
    if (range.x >= range.y) return;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];

    // Per-pixel state.  Algebra: with dotc = sum_c color_c * v_out_c (per pixel x Gaussian)
    // and bv = sum_c buffer_c * v_out_c (maintained incrementally: bv += fac * dotc), upstream's
    //   v_alpha = sum_c (color_c*T - buffer_c*ra) * v_out_c + T_final*ra*v_out_alpha - T_final*ra*sum_c bg_c*v_out_c
    // becomes  v_alpha = ra * (T_before * dotc - bv + c0),  c0 = T_final * (v_out_alpha - sum_c bg_c*v_out_c),
    // i.e. 3 VALU ops instead of ~26, one running scalar instead of a 3-channel buffer.
    float px[QPW], py[QPW], T[QPW], c0[QPW], bv[QPW], vo0[QPW], vo1[QPW], vo2[QPW];
    int kfin[QPW], pixi[QPW];
    int kmax_l = -1;
#pragma unroll
    for (int q = 0; q < QPW; ++q) {          // phase 1: where does each pixel's walk start?
        int ox, oy;
        bool in_tile;
        slot_pixel(q0 + q, lane, B, ox, oy, in_tile);
        const int j = tx * B + ox, i = ty * B + oy;
        const bool inside = in_tile && j < W && i < H;
        pixi[q] = inside ? i * W + j : -1;
        px[q] = (float)j + 0.5f;
        py[q] = (float)i + 0.5f;
        kfin[q] = inside ? final_idx[pixi[q]] : -1;  // -1: this slot never participates
        kmax_l = max(kmax_l, kfin[q]);
    }
    int kmax = __builtin_amdgcn_readfirstlane(wave_max_i(kmax_l));
    kmax = min(kmax, range.y - 1);
    if (kmax < range.x) return;
    if constexpr (ADAPT) {                   // split tiles whose reverse walk is long, one quadrant per wave
        const bool split = (kmax - range.x + 1) >= adapt_thresh;
        if (!split && wv != 0) return;
        if (split) {
            int km = -1;
#pragma unroll
            for (int q = 0; q < QPW; ++q) {
                if (q != wv) { kfin[q] = -1; pixi[q] = -1; } else km = kfin[q];
            }
            kmax = min(__builtin_amdgcn_readfirstlane(wave_max_i(km)), range.y - 1);
            if (kmax < range.x) return;
        }
    }
#pragma unroll
    for (int q = 0; q < QPW; ++q) {          // phase 2: per-pixel state of the active slots
        const bool inside = pixi[q] >= 0;
        const int pix = inside ? pixi[q] : 0;
        const float Tf = inside ? final_T[pix] : 1.f;
        T[q] = Tf;
        // A pixel nothing was composited onto (its transmittance stayed EXACTLY 1: the first composited entry makes it
        // <= 254/255) takes no part in the reverse walk; upstream never reads its incoming gradients.  The body below is
        // branch-free — a masked lane contributes `0 * v_out` — so a non-finite value there would reach the sums as
        // 0 x NaN.  Such values are ordinary: `depth / alpha` under a `where(alpha > eps, ...)` (sgn_splatfacto.py:995)
        // has gradient 0 / 0 on every uncovered pixel.  Their gradients are therefore not loaded at all (round 5).
        const bool live = inside && Tf < 1.f;
        // v_out == NULL: the image took no part in the loss (an accumulation-only pass): zeros, and no 29 MB read
        vo0[q] = (live && v_out != nullptr) ? v_out[3 * pix] : 0.f;
        vo1[q] = (live && v_out != nullptr) ? v_out[3 * pix + 1] : 0.f;
        vo2[q] = (live && v_out != nullptr) ? v_out[3 * pix + 2] : 0.f;
        const float voa = live ? v_out_alpha[pix] : 0.f;
        c0[q] = Tf * (voa - fmaf(bg0, vo0[q], fmaf(bg1, vo1[q], bg2 * vo2[q])));
        bv[q] = 0.f;
    }

    const bool qtest = (B == 16);
    const float qcx = (float)(tx * 16 + (lane & 1) * 8) + 4.0f, qcy = (float)(ty * 16 + ((lane >> 1) & 1) * 8) + 4.0f;
    bool kfin_active[QPW];   // wave-uniform: does any pixel of this slot take part in the reverse walk?
#pragma unroll
    for (int q = 0; q < QPW; ++q) kfin_active[q] = __ballot(kfin[q] >= range.x) != 0ull;

    // one depth-list entry (reverse walk) for this wave's pixels
    auto entry = [&](const Rec &cur, int k, unsigned qm) __attribute__((always_inline)) {
        // Spatial terms as raw MOMENTS (r03): m = sum vs (dx, dy), s = sum vs (dx^2, dx dy, dy^2).  The conic that turns
        // them into v_xy = (a m_x + b m_y, b m_x + c m_y) and v_conic = (s_xx / 2, s_xy, s_yy / 2) is a per-GAUSSIAN
        // constant, so it is applied once per Gaussian in unpack_grads_kernel instead of once per (pixel, entry) here:
        // 2 mul + 2 add + 3 fma in place of 4 mul + 7 fma.
        float m_x = 0.f, m_y = 0.f, s_xx = 0.f, s_xy = 0.f, s_yy = 0.f;
        float g_r = 0.f, g_g = 0.f, g_b = 0.f, g_o = 0.f;
        float ax = 0.f, ay = 0.f, cA = 0.f, cC = 0.f;     // ABSGRAD: the absolute sums, the entry's un-halved conic
        if constexpr (ABSGRAD) { cA = cur.ha + cur.ha; cC = cur.hc + cur.hc; }
        bool any = false;
#pragma unroll
        for (int q = 0; q < QPW; ++q) {
            if (!((qm >> (q0 + q)) & 1u) || __ballot(k <= kfin[q]) == 0ull) continue;  // wave-uniform
            const float dx = cur.x - px[q], dy = cur.y - py[q];
            const float t1 = cur.ha * dx, t2 = cur.hc * dy, t3 = cur.b * dx;
            const float sigma = fmaf(t3, dy, fmaf(t2, dy, t1 * dx));
            const float vis = sgn_exp<EXACT>(-sigma);
            const float av = cur.opac * vis;
            const float alpha = fminf(alpha_clamp, av);
            const bool valid = (k <= kfin[q]) && sigma >= 0.f && alpha >= (1.f / 255.f);
            // branch-free: everything is evaluated, invalid lanes are masked out by three selects.  (ONE select — an
            // invalid lane continuing with vis = 0, so that alpha = 0, ra = 1, fac = 0, vs = 0 — was measured in r03:
            // 3 % SLOWER on all three workloads; the select then sits in front of the rcp on the dependency chain.)
            const float ra = __builtin_amdgcn_rcpf(1.f - alpha);   // v_rcp_f32 (1 ulp); oracle divides exactly
            const float Tn = T[q] * ra;
            const float fac = alpha * Tn;
            const float dotc = fmaf(cur.r, vo0[q], fmaf(cur.g, vo1[q], cur.bl * vo2[q]));
            const float v_alpha = ra * fmaf(T[q], dotc, c0[q] - bv[q]);
            const float vm = valid ? v_alpha : 0.f;
            const float facm = valid ? fac : 0.f;
            bv[q] = fmaf(facm, dotc, bv[q]);
            T[q] = valid ? Tn : T[q];
            const float vs = -av * vm;                              // v_sigma (upstream: not zeroed by the clamp)
            const float p = vs * dx, qq = vs * dy;
            m_x += p;
            m_y += qq;
            s_xx = fmaf(p, dx, s_xx);
            s_xy = fmaf(p, dy, s_xy);
            s_yy = fmaf(qq, dy, s_yy);
            if constexpr (ABSGRAD) {
                ax += fabsf(fmaf(cA, p, cur.b * qq));
                ay += fabsf(fmaf(cur.b, p, cC * qq));
            }
            g_r = fmaf(facm, vo0[q], g_r);
            g_g = fmaf(facm, vo1[q], g_g);
            g_b = fmaf(facm, vo2[q], g_b);
            g_o = fmaf(vis, vm, g_o);
            any = any || valid;
        }
        if (__ballot(any) != 0ull) {  // wave-uniform
            if constexpr (REDUCE == 1) {
                float t0 = fold16(fold32(m_x, m_y), fold32(s_xx, s_xy));     // rows: m_x, s_xx, m_y, s_xy
                float t1 = fold16(fold32(s_yy, g_r), fold32(g_g, g_b));      // rows: s_yy, g, r, b
                float t2;
                if constexpr (ABSGRAD) t2 = fold16(fold32(g_o, ax), fold32(ay, 0.f));   // rows: o, ay, ax, 0
                else t2 = fold16(fold32(g_o, 0.f), 0.f);                     // rows: o, 0, 0, 0
                t0 = row_sum_dpp(t0); t1 = row_sum_dpp(t1); t2 = row_sum_dpp(t2);
                const int c = lane & 15, row = lane >> 4;
                const int rowmap = ((row & 1) << 1) | (row >> 1);            // rows 0,1,2,3 hold values 0,2,1,3
                const float mine = (c == 0) ? t0 : (c == 1) ? t1 : t2;
                // (ABSGRAD: column 2 of rows 0, 1, 2 = slots 8, 10, 9)
                if ((c < 2 || (ABSGRAD ? (c == 2 && row < 3) : lane == 2)) && !(dbg & 1))
                    unsafeAtomicAdd(grad_ws + (size_t)cur.gid * SGN_RECORD_FLOATS + (c * 4 + rowmap), mine);
            } else {
                if (!(dbg & 2)) {          // dbg bit1: ablation only, skip the wave reduction (results are wrong)
                    m_x = wave_sum(m_x); m_y = wave_sum(m_y);
                    s_xx = wave_sum(s_xx); s_xy = wave_sum(s_xy); s_yy = wave_sum(s_yy);
                    g_r = wave_sum(g_r); g_g = wave_sum(g_g); g_b = wave_sum(g_b);
                    g_o = wave_sum(g_o);
                    if constexpr (ABSGRAD) { ax = wave_sum(ax); ay = wave_sum(ay); }
                }
                float mine = m_x;
                mine = (lane == 1) ? m_y : mine;
                mine = (lane == 2) ? s_xx : mine;
                mine = (lane == 3) ? s_xy : mine;
                mine = (lane == 4) ? s_yy : mine;
                mine = (lane == 5) ? g_r : mine;
                mine = (lane == 6) ? g_g : mine;
                mine = (lane == 7) ? g_b : mine;
                mine = (lane == 8) ? g_o : mine;
                if constexpr (ABSGRAD) {
                    mine = (lane == 9) ? ax : mine;
                    mine = (lane == 10) ? ay : mine;
                }
                if (lane < (ABSGRAD ? 11 : 9) && !(dbg & 1))  // dbg bit0: ablation, no atomics
                    unsafeAtomicAdd(grad_ws + (size_t)cur.gid * SGN_RECORD_FLOATS + lane, mine);
            }
        }
    };

    // the reverse walk, kmax down to range.x: the forward's two ways through the list, downwards
    const int L = kmax - range.x + 1;
    if (L < batch_thresh) {
        walk_chase<-1, false>(ids, recs, nullptr, idmask, kmax, range.x, [&](const Rec &cur, int raw, int k, float) {
            entry(cur, k, qm_on ? qm_bits(raw, cur.ex) : quadrant_mask(cur, qcx, qcy, qtest));
            return true;
        });
    } else {
        __shared__ float4 stage[2][64 * 3];
        unsigned mine_q = 0u;
#pragma unroll
        for (int q = 0; q < QPW; ++q)
            if (kfin_active[q]) mine_q |= 1u << (q0 + q);
        walk_staged<-1, false>(
            ids, recs, nullptr, idmask, kmax, L, stage, nullptr,
            [&](int raw, const float4 &r0, const float4 &r2) {
                return (qm_on ? qm_bits(raw, r2.z) : row_quadrants(r0.x, r0.y, r2.z, r2.w, tx * 16, ty * 16, qtest)) & mine_q;
            },
            [](bool, int) {},
            [&](const Rec &cur, int, int k, unsigned qm, float) {
                entry(cur, k, qm);
                return true;
            });
    }
}

// row i of the four gradient arrays from its row of the packed gradient workspace (a, b, c = the row's three float4)
__device__ __forceinline__ void unpack_row(int i, const float4 &a, const float4 &b, const float4 &c,
                                           const float *__restrict__ conics, const float *__restrict__ opac,
                                           int opac_is_logit, const float *__restrict__ colors_pre,
                                           float *__restrict__ v_xy, float *__restrict__ v_conic,
                                           float *__restrict__ v_colors, float *__restrict__ v_opac) {
    moments_to_grads(conics + 3 * i, a, b.x, v_xy + 2 * i, v_conic + 3 * i);
    float v0 = b.y, v1 = b.z, v2 = b.w;
    if (colors_pre != nullptr) {   // the colours were clamp(pre, min = 0): gradient w.r.t. `pre` (torch: grad * (pre >= 0))
        v0 = colors_pre[3 * i] >= 0.f ? v0 : 0.f;
        v1 = colors_pre[3 * i + 1] >= 0.f ? v1 : 0.f;
        v2 = colors_pre[3 * i + 2] >= 0.f ? v2 : 0.f;
    }
    v_colors[3 * i] = v0; v_colors[3 * i + 1] = v1; v_colors[3 * i + 2] = v2;
    float vo = c.x;
    if (opac_is_logit == 1) {         // opac holds logits: chain through the fused sigmoid
        const float sg = 1.f / (1.f + expf(-opac[i]));
        vo = vo * sg * (1.f - sg);
    } else if (opac_is_logit == 2) {  // opac holds sigmoid OUTPUTS, the gradient w.r.t. their logits is wanted
        const float sg = opac[i];
        vo = vo * sg * (1.f - sg);
    }
    v_opac[i] = vo;
}

// Kernel-selection options arrive with every call (include/sgn_rast.h: sgn_raster_opts); NULL = defaults.
inline sgn_raster_opts resolve_opts(const sgn_raster_opts *o) {
    sgn_raster_opts r;
    sgn_raster_default_opts(&r);
    if (o) {
        r = *o;
        r.exact_exp = r.exact_exp ? 1 : 0;
        r.reduce_mode = r.reduce_mode ? 1 : 0;
        r.ids_qmask = r.ids_qmask ? 1 : 0;
        sgn_raster_opts d;
        sgn_raster_default_opts(&d);
        if (r.adapt_fwd <= 0) r.adapt_fwd = d.adapt_fwd;
        if (r.adapt_bwd <= 0) r.adapt_bwd = d.adapt_bwd;
        if (r.batch_fwd <= 0) r.batch_fwd = d.batch_fwd;
        if (r.batch_bwd <= 0) r.batch_bwd = d.batch_bwd;
    }
    return r;
}

// ---- host side of the reverse walks.  Every backward kernel (raster.hip plain and batched views, raster_absgrad.hip)
// has this parameter list; only the third and fourth int differ in meaning: (B, tiles_x) for a single view,
// (tiles_x, tiles_per_view) for batched views.
using RasterBwdKernel = void (*)(int W, int H, int i2, int i3, int n_tiles, const int2 *bins, const Rec *recs,
                                 const int32_t *ids, const float *bg, const float *final_T, const int32_t *final_idx,
                                 const float *v_out, const float *v_out_alpha, float alpha_clamp, float *grad_ws, int dbg,
                                 int adapt_thresh, int batch_thresh, const int32_t *tile_order, int use_qm);
// A family's launch shapes (raster.hip "Launch shapes of the backward"), each [exact_exp][reduce_mode]; every unit
// defines the table of its own kernels.  adaptive == nullptr: the family always runs the two-kernel scheme.
struct RasterBwdFamily {
    RasterBwdKernel adaptive[2][2];     // the in-kernel adaptive split: no launch order / tiles other than 16x16
    RasterBwdKernel long_walk[2][2];    // two-kernel scheme: order[0..n_long), four lean waves per tile
    RasterBwdKernel short_walk[2][2];   //                    the rest, one wave per tile
};
// the kernel arguments; n_tiles is also the launch grid's tile count, o the resolved options
struct RasterBwdArgs {
    int W, H, i2, i3, n_tiles;
    const int2 *bins;
    const Rec *recs;
    const int32_t *ids;
    const float *bg, *final_T;
    const int32_t *final_idx;
    const float *v_out, *v_out_alpha;
    float alpha_clamp;
    float *grad_ws;
    const int32_t *tile_order;
    sgn_raster_opts o;
};
// what sgn_raster_bwd, sgn_raster_bwd_part and sgn_raster_bwd_abs are called with (include/sgn_rast.h)
struct RasterBwdCall {
    int img_h, img_w, block_width, n;
    int64_t n_isect;
    const int32_t *gaussian_ids_sorted, *tile_bins;
    const float *xys, *conics, *colors, *opacities;
    int opacity_is_logit, id_lo, id_hi, window;
    const float *background3, *final_Ts;
    const int32_t *final_idx;
    const float *v_out_img, *v_out_alpha;
    float alpha_clamp_bwd;
    float *v_xy, *v_conic, *v_colors, *v_opacity;
    void *recs_ws;
    size_t recs_ws_bytes;
    int recs_packed;
    void *grad_ws;
    size_t grad_ws_bytes;
    const int32_t *tile_order;
    const float *colors_pre_clamp;
    const sgn_raster_opts *opts;
    sgn_stream_t stream, aux_stream;
};

}  // namespace

// Both defined in raster.hip.  C linkage: Rec and the types above live in each unit's unnamed namespace (the kernels'
// symbols carry it), so a C++ function over them could not be defined in another unit; the layouts are one header's.
// sgn_raster_bwd_launch: fork to `aux` (two_kernel, aux lent and not `s`, events available), SGN_T_RASTER_BWD, the
// family's kernels for a.o — adaptive on s (grid 4 * n_tiles), or long_walk on aux (4 * n_tiles) then short_walk on s
// (n_tiles) — and the join.
extern "C" int sgn_raster_bwd_launch(const RasterBwdFamily *family, const RasterBwdArgs *a, int two_kernel,
                                     hipStream_t s, hipStream_t aux);
// sgn_raster_bwd_walks: the single-view entries up to their unpack — the argument checks (reported under `fn`), the
// workspace clear (clear_ws), the row build (unless c.recs_packed) and, n_isect > 0, the launch.  n == 0: nothing queued.
extern "C" int sgn_raster_bwd_walks(const char *fn, const RasterBwdFamily *family, const RasterBwdCall *c,
                                    int clear_ws);
