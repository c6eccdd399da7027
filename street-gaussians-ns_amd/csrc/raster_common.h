// Per-entry helpers shared by the raster translation units (raster.hip, raster_layers.hip): the 48-byte row, the two
// exp forms and the quadrant tests.  Moved here unchanged from raster.hip; the arithmetic contract is in its header.
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

}  // namespace
