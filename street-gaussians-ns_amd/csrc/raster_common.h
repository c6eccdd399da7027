// What the raster translation units (raster.hip, raster_layers.hip, raster_features.hip) share: the 48-byte row, the two
// exp forms, the quadrant tests, the wave helpers (maximum, the transposed permlane-swap reduction), the per-Gaussian
// arithmetic around the walks (the alpha >= 1/255 box, moments -> gradients), the block -> (tile, wave) map of the packed
// launch, and the two ways through a depth list — walk_chase and walk_staged.  A kernel supplies what it does per entry
// (and per batch); the traversal, with its prefetch discipline, is written here once.  The arithmetic contract is in
// raster.hip's header; all three units are built with -ffp-contract=off -fno-slp-vectorize, so shared source gives the
// same bits in each.
#pragma once
#include "sgn_common.h"

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

}  // namespace
