// sh.hip — view-dependent colour from real spherical harmonics (forward + backward), gfx950.
//
// Replaces gsplat 0.1.x sh.cuh compute_sh_forward_kernel / compute_sh_backward_kernel
// (method="fast", Sloan recurrences), reached from the reference at
// sgn_splatfacto.py:939 and sgn_splatfacto_scene_graph.py:285.
//
// Pure streaming, HBM-bound: 12 B dir + 12*K B coeffs -> 12 B colour per Gaussian (216 B at K=16).
// Layout trick for 64-wide waves: the [n,K,3] coefficient block of 64 consecutive Gaussians is one
// contiguous 64*K*12-byte span, so each wave copies its span to LDS with full-width
// global_load_dwordx4 (lane-contiguous, every byte of every cache line used once) and then each
// lane walks its own K*3 row from LDS; the row stride (3K+1 dwords) is odd, so the 64 lanes hit
// distinct banks.  The backward writes v_coeffs the same way in reverse (row -> LDS -> coalesced
// dwordx4 stores).
//
// Five kernel families (plain, fused front end, un-concatenated sub-models, multi-view backward, batched views) share
// the per-row helpers below: the families that promise each other equal bits run the same source operations in the
// same order (-ffp-contract=off), because they call the same code.
#include <type_traits>

#include "sgn_common.h"

namespace {

__device__ __forceinline__ int sh_bases(float dx, float dy, float dz, int deg, float *b) {
    b[0] = 0.2820947917738781f;
    if (deg < 1) return 1;
    const float inorm = 1.f / sqrtf(dx * dx + dy * dy + dz * dz);
    const float x = dx * inorm, y = dy * inorm, z = dz * inorm;
    const float fTmp0A = 0.48860251190292f;
    b[1] = -fTmp0A * y; b[2] = fTmp0A * z; b[3] = -fTmp0A * x;
    if (deg < 2) return 4;
    const float z2 = z * z;
    const float fTmp0B = -1.092548430592079f * z;
    const float fTmp1A = 0.5462742152960395f;
    const float fC1 = x * x - y * y;
    const float fS1 = 2.f * x * y;
    b[6] = 0.9461746957575601f * z2 - 0.3153915652525201f;
    b[7] = fTmp0B * x; b[5] = fTmp0B * y; b[8] = fTmp1A * fC1; b[4] = fTmp1A * fS1;
    if (deg < 3) return 9;
    const float fTmp0C = -2.285228997322329f * z2 + 0.4570457994644658f;
    const float fTmp1B = 1.445305721320277f * z;
    const float fTmp2A = -0.5900435899266435f;
    const float fC2 = x * fC1 - y * fS1;
    const float fS2 = x * fS1 + y * fC1;
    b[12] = z * (1.865881662950577f * z2 - 1.119528997770346f);
    b[13] = fTmp0C * x; b[11] = fTmp0C * y; b[14] = fTmp1B * fC1; b[10] = fTmp1B * fS1;
    b[15] = fTmp2A * fC2; b[9] = fTmp2A * fS2;
    if (deg < 4) return 16;
    const float fTmp0D = z * (-4.683325804901025f * z2 + 2.007139630671868f);
    const float fTmp1C = 3.31161143515146f * z2 - 0.47308734787878f;
    const float fTmp2B = -1.770130769779931f * z;
    const float fTmp3A = 0.6258357354491763f;
    const float fC3 = x * fC2 - y * fS2;
    const float fS3 = x * fS2 + y * fC2;
    b[20] = 1.984313483298443f * z * b[12] + -1.006230589874905f * b[6];
    b[21] = fTmp0D * x; b[19] = fTmp0D * y; b[22] = fTmp1C * fC1; b[18] = fTmp1C * fS1;
    b[23] = fTmp2B * fC2; b[17] = fTmp2B * fS2; b[24] = fTmp3A * fC3; b[16] = fTmp3A * fS3;
    return 25;
}

// ---- stage-in: a wave's contiguous coefficient rows -> its LDS slab --------------------------------------------------
// The two halves of the aligned copy, separate so that the loads of the NEXT span can be in flight while this one is
// evaluated (sh_fwd_kernel).  ALL global loads are issued before the first LDS write: written as a plain
// `for (t...) { load; store }` loop the compiler emits load -> s_waitcnt vmcnt(0) -> ds_write per iteration, i.e. 12
// serialised HBM round trips per wave (sh_fwd: 68 us -> see DESIGN.md).
template <int KC>
__device__ __forceinline__ void load_span(float4 (&v)[(16 * KC + 63) / 64], const float *__restrict__ src, int cnt,
                                          int lane) {
    constexpr int NIT = (16 * KC + 63) / 64;          // float4 loads per lane for a full wave of 64 rows
    const int n4 = (cnt * KC) >> 2;
    const float4 *src4 = reinterpret_cast<const float4 *>(src);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int t = lane + 64 * it;
        v[it] = (t < n4) ? src4[t] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
template <int KC, int LS>
__device__ __forceinline__ void store_span(float *__restrict__ my, const float4 (&v)[(16 * KC + 63) / 64],
                                           const float *__restrict__ src, int cnt, int lane) {
    constexpr int NIT = (16 * KC + 63) / 64;
    const int total = cnt * KC, n4 = total >> 2;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int t = lane + 64 * it;
        if (t < n4) {
            const float f[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * t + j, r = e / KC, c = e - r * KC;
                my[r * LS + c] = f[j];
            }
        }
    }
    const int e = (n4 << 2) + lane;                   // up to three trailing floats of a partial wave
    if (lane < (total & 3)) {
        const int r = e / KC, c = e - r * KC;
        my[r * LS + c] = src[e];
    }
}

// Copy this wave's `cnt` contiguous coefficient rows (KC floats each) into its LDS slab with row stride LS.
template <int KC, int LS>
__device__ __forceinline__ void stage_rows(float *__restrict__ my, const float *__restrict__ src, int cnt, int lane) {
    const int total = cnt * KC;
    if (reinterpret_cast<uintptr_t>(src) & 15) {      // a view with an odd storage offset: plain dword copy
        for (int e = lane; e < total; e += 64) {
            const int r = e / KC, c = e - r * KC;
            my[r * LS + c] = src[e];
        }
        return;
    }
    float4 v[(16 * KC + 63) / 64];
    load_span<KC>(v, src, cnt, lane);
    store_span<KC, LS>(my, v, src, cnt, lane);
}

// LDS traffic between lanes of ONE wave (private slab): the hardware retires a wave's LDS operations in order, the
// fence only keeps the compiler from moving them across
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- drain: the wave's LDS rows -> `cnt` contiguous global rows of W floats -----------------------------------------
// Row r of the slab starts at my + r * LS; its columns C0 .. C0 + W - 1 go out.  VEC4 (W % 4 == 0 and a 16-byte
// aligned dst) stores float4, otherwise one dword per lane.
template <int W, int LS, int C0, bool VEC4>
__device__ __forceinline__ void drain_rows(float *dst, const float *my, int cnt, int lane) {
    const int total = cnt * W;
    if constexpr (VEC4) {
        float4 *dst4 = reinterpret_cast<float4 *>(dst);
        for (int t = lane; t < total / 4; t += 64) {
            const int e = t * 4, r = e / W, c = e - r * W;
            const float *s = my + r * LS + C0 + c;
            dst4[t] = make_float4(s[0], s[1], s[2], s[3]);
        }
    } else {
        for (int e = lane; e < total; e += 64) {
            const int r = e / W, c = e - r * W;
            dst[e] = my[r * LS + C0 + c];
        }
    }
}
// Rows of KC floats, split over the two leaves of the reference: band 0 -> v_dc [n,3], the rest -> v_rest [n,K-1,3].
template <int KC, int LS>
__device__ __forceinline__ void drain_dc_rest(float *v_dc, float *v_rest, int g0, const float *my, int cnt, int lane) {
    drain_rows<3, LS, 0, false>(v_dc + (size_t)g0 * 3, my, cnt, lane);
    if constexpr (KC > 3) drain_rows<KC - 3, LS, 3, false>(v_rest + (size_t)g0 * (KC - 3), my, cnt, lane);
}

// ---- per-row arithmetic ---------------------------------------------------------------------------------------------
// local -> world by one 16-float pose row (scene_graph.py:414)
__device__ __forceinline__ void pose_apply(const float *P, float &m0, float &m1, float &m2) {
    const float w0 = P[0] * m0 + P[1] * m1 + P[2] * m2 + P[9];
    const float w1 = P[3] * m0 + P[4] * m1 + P[5] * m2 + P[10];
    const float w2 = P[6] * m0 + P[7] * m1 + P[8] * m2 + P[11];
    m0 = w0; m1 = w1; m2 = w2;
}

__device__ __forceinline__ void fused_viewdir(int i, const float *__restrict__ means,
                                              const float *__restrict__ cam_pos,
                                              const int32_t *__restrict__ object_ids,
                                              const float *__restrict__ poses, float &dx, float &dy, float &dz) {
    float m0 = means[3 * i], m1 = means[3 * i + 1], m2 = means[3 * i + 2];
    if (poses != nullptr && object_ids != nullptr) pose_apply(poses + 16 * (size_t)object_ids[i], m0, m1, m2);
    dx = m0 - cam_pos[0]; dy = m1 - cam_pos[1]; dz = m2 - cam_pos[2];
}

// Effective DC term of one row, dc_eff = sum_f dc[f, :] * w[f] from 0.f in ascending f (Fourier "4D-SH" DC term,
// sgn_splatfacto_scene_graph.py:239-247).  `w` is anything indexable; the batched views pass ShUnitWeight with F = 1,
// which performs 0.f + dc * 1.f and NOT just `dc`: the sum turns a -0.f into +0.f, as the fused kernel's does.
struct ShUnitWeight {
    __device__ __forceinline__ float operator[](int) const { return 1.f; }
};
template <class Weights>
__device__ __forceinline__ void sh_dc_eff(const float *dc, int F, Weights w, float &d0, float &d1, float &d2) {
    d0 = 0.f; d1 = 0.f; d2 = 0.f;
    for (int f = 0; f < F; ++f) {
        const float wf = w[f];
        d0 += dc[3 * f] * wf; d1 += dc[3 * f + 1] * wf; d2 += dc[3 * f + 2] * wf;
    }
}
// ... and its backward: v_dc[f, :] = (w[f] * b0) * v
__device__ __forceinline__ void sh_dc_fan_out(float *v_dc, int F, const float *w, float b0, float v0, float v1,
                                              float v2) {
    for (int f = 0; f < F; ++f) {
        const float wf = w[f] * b0;
        v_dc[3 * f] = wf * v0; v_dc[3 * f + 1] = wf * v1; v_dc[3 * f + 2] = wf * v2;
    }
}

// (a0, a1, a2) += bands K0 .. K-1 dotted with an LDS row whose first entry is band K0
template <int K0, int K>
__device__ __forceinline__ void sh_eval_bands(const float *b, int nb, const float *row, float &a0, float &a1,
                                              float &a2) {
#pragma unroll
    for (int k = K0; k < K; ++k) {
        if (k < nb) {
            a0 += b[k] * row[3 * (k - K0)];
            a1 += b[k] * row[3 * (k - K0) + 1];
            a2 += b[k] * row[3 * (k - K0) + 2];
        }
    }
}
// the post step clamp(x + 0.5, min=0) and its backward: the gradient passes where the output `c` is positive
__device__ __forceinline__ void sh_post(float &a0, float &a1, float &a2) {
    a0 = fmaxf(a0 + 0.5f, 0.f); a1 = fmaxf(a1 + 0.5f, 0.f); a2 = fmaxf(a2 + 0.5f, 0.f);
}
__device__ __forceinline__ void sh_post_gate(const float *c, float &v0, float &v1, float &v2) {
    v0 = c[0] > 0.f ? v0 : 0.f;
    v1 = c[1] > 0.f ? v1 : 0.f;
    v2 = c[2] > 0.f ? v2 : 0.f;
}

// backward of one row: bands K0 .. K-1 of b[k] * v (zero above the active degree) into an LDS row that starts at K0 ...
template <int K0, int K>
__device__ __forceinline__ void sh_fill_row(float *row, const float *b, int nb, float v0, float v1, float v2) {
#pragma unroll
    for (int k = K0; k < K; ++k) {
        const float bk = (k < nb) ? b[k] : 0.f;
        row[3 * (k - K0)] = bk * v0; row[3 * (k - K0) + 1] = bk * v1; row[3 * (k - K0) + 2] = bk * v2;
    }
}
// ... or summed over views into registers
template <int K>
__device__ __forceinline__ void sh_accumulate(float (&acc)[3 * K], const float *b, int nb, float v0, float v1,
                                              float v2) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float bk = (k < nb) ? b[k] : 0.f;
        acc[3 * k] += bk * v0; acc[3 * k + 1] += bk * v1; acc[3 * k + 2] += bk * v2;
    }
}

// ---- plain SH ---------------------------------------------------------------------------------------------------------
// One wave (64 lanes) per span of 64 Gaussians; a block is WAVES waves with private LDS slabs and each wave walks
// spans in a grid-stride loop with the NEXT span's twelve float4 loads already in flight while it evaluates the
// current one (one span per wave and no prefetch reached 4.1 TB/s where a plain streaming read on this GPU reaches
// 6.5, profiles/microbench/hbm_rates.hip: with 12.5 KB of LDS per wave only 12 waves fit a CU, and each spent most
// of its life NOT waiting for memory).
// KC = K*3 dwords per row; LDS row stride KC+1 (odd) => conflict-free per-lane row walks.
template <int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sh_fwd_kernel(int n, int deg, const float *__restrict__ dirs,
                                                            const float *__restrict__ coeffs,
                                                            float *__restrict__ colors) {
    constexpr int KC = K * 3, LS = KC + 1, NIT = (16 * KC + 63) / 64;
    __shared__ float lds[WAVES][64 * LS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n_spans = (n + 63) >> 6, stride = gridDim.x * WAVES;
    float *my = lds[wave];
    const bool aligned = (reinterpret_cast<uintptr_t>(coeffs) & 15) == 0;   // 64 rows * KC floats keep the alignment
    int span = blockIdx.x * WAVES + wave;
    float4 v[NIT];
    float d0 = 0.f, d1 = 0.f, d2 = 1.f;               // this lane's view direction of the span in flight
    auto fetch = [&](int sp) __attribute__((always_inline)) {
        const int g = sp * 64, c = min(64, n - g);
        if (aligned) load_span<KC>(v, coeffs + (size_t)g * KC, c, lane);
        if (lane < c) { d0 = dirs[3 * (g + lane)]; d1 = dirs[3 * (g + lane) + 1]; d2 = dirs[3 * (g + lane) + 2]; }
    };
    if (span < n_spans) fetch(span);
    for (; span < n_spans; span += stride) {
        const int g0 = span * 64, cnt = min(64, n - g0);
        const float *src = coeffs + (size_t)g0 * KC;
        if (aligned) store_span<KC, LS>(my, v, src, cnt, lane);
        else stage_rows<KC, LS>(my, src, cnt, lane);                        // a view with an odd storage offset
        const float x = d0, y = d1, z = d2;
        const int next = span + stride;
        if (next < n_spans) fetch(next);
        wave_lds_fence();
        if (lane < cnt) {
            const int i = g0 + lane;
            float b[25];
            const int nb = sh_bases(x, y, z, deg, b);
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            sh_eval_bands<0, K>(b, nb, my + lane * LS, a0, a1, a2);
            colors[3 * i] = a0; colors[3 * i + 1] = a1; colors[3 * i + 2] = a2;
        }
        wave_lds_fence();                              // this span's row reads stay ahead of the next span's writes
    }
}

template <int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sh_bwd_kernel(int n, int deg, const float *__restrict__ dirs,
                                                            const float *__restrict__ v_colors,
                                                            float *__restrict__ v_coeffs) {
    constexpr int KC = K * 3, LS = KC + 1;
    __shared__ float lds[WAVES][64 * LS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (blockIdx.x * WAVES + wave) * 64;
    const int cnt = max(0, min(64, n - g0));
    float *my = lds[wave];
    if (lane < cnt) {
        const int i = g0 + lane;
        float b[25];
        const int nb = sh_bases(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], deg, b);
        sh_fill_row<0, K>(my + lane * LS, b, nb, v_colors[3 * i], v_colors[3 * i + 1], v_colors[3 * i + 2]);
    }
    __syncthreads();
    drain_rows<KC, LS, 0, KC % 4 == 0>(v_coeffs + (size_t)g0 * KC, my, cnt, lane);
}

// ---- fused SH front end (extension) ------------------------------------------------
// colour = clamp( SH(deg, means - cam_pos, [dc_eff | rest]) + 0.5, min 0 )  with
// dc_eff = sum_f features_dc[:, f, :] * idft[object, f]   (F = 1 and idft = [1] for the background model).
// Replaces, per call: view-dir subtract + norm + divide, the Fourier sum, torch.cat((dc, rest)) (192 MB at
// 1 M Gaussians), the SH op, +0.5 and clamp — and the matching backward kernels — by one pass.
// Here and below KC = (K-1)*3 dwords of features_rest per row, LDS row stride KC | 1 (odd).
template <int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sh_fwd_fused_kernel(
    int n, int deg, const float *__restrict__ means, const float *__restrict__ cam_pos,
    const float *__restrict__ dc, int F, const float *__restrict__ rest, const int32_t *__restrict__ object_ids,
    const float *__restrict__ idft, const float *__restrict__ poses, int post, float *__restrict__ colors) {
    constexpr int KC = (K - 1) * 3, LS = (KC | 1);
    __shared__ float lds[WAVES][64 * (KC > 0 ? LS : 1)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (blockIdx.x * WAVES + wave) * 64;
    const int cnt = max(0, min(64, n - g0));
    float *my = lds[wave];
    if constexpr (KC > 0) stage_rows<KC, LS>(my, rest + (size_t)g0 * KC, cnt, lane);
    __syncthreads();
    if (lane >= cnt) return;
    const int i = g0 + lane;
    float b[25];
    float vx, vy, vz;
    fused_viewdir(i, means, cam_pos, object_ids, poses, vx, vy, vz);
    const int nb = sh_bases(vx, vy, vz, deg, b);
    float d0, d1, d2;
    sh_dc_eff(dc + (size_t)i * F * 3, F, idft + (size_t)(object_ids ? object_ids[i] : 0) * F, d0, d1, d2);
    float a0 = b[0] * d0, a1 = b[0] * d1, a2 = b[0] * d2;
    sh_eval_bands<1, K>(b, nb, my + lane * LS, a0, a1, a2);
    if (post) sh_post(a0, a1, a2);
    colors[3 * i] = a0; colors[3 * i + 1] = a1; colors[3 * i + 2] = a2;
}

template <int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sh_bwd_fused_kernel(
    int n, int deg, const float *__restrict__ means, const float *__restrict__ cam_pos, int F,
    const int32_t *__restrict__ object_ids, const float *__restrict__ idft, const float *__restrict__ poses,
    int post, const float *__restrict__ colors, const float *__restrict__ v_colors, float *__restrict__ v_dc,
    float *__restrict__ v_rest) {
    constexpr int KC = (K - 1) * 3, LS = (KC | 1);
    __shared__ float lds[WAVES][64 * (KC > 0 ? LS : 1)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (blockIdx.x * WAVES + wave) * 64;
    const int cnt = max(0, min(64, n - g0));
    float *my = lds[wave];
    if (lane < cnt) {
        const int i = g0 + lane;
        float b[25];
        float vx, vy, vz;
        fused_viewdir(i, means, cam_pos, object_ids, poses, vx, vy, vz);
        const int nb = sh_bases(vx, vy, vz, deg, b);
        float v0 = v_colors[3 * i], v1 = v_colors[3 * i + 1], v2 = v_colors[3 * i + 2];
        if (post) sh_post_gate(colors + 3 * i, v0, v1, v2);
        sh_dc_fan_out(v_dc + (size_t)i * F * 3, F, idft + (size_t)(object_ids ? object_ids[i] : 0) * F, b[0], v0, v1,
                      v2);
        sh_fill_row<1, K>(my + lane * LS, b, nb, v0, v1, v2);
    }
    __syncthreads();
    if constexpr (KC > 0) drain_rows<KC, LS, 0, false>(v_rest + (size_t)g0 * KC, my, cnt, lane);
}

// ---- fused SH over UN-CONCATENATED sub-models (round 4) ---------------------------------------------------------------
// The scene graph keeps one `features_dc` / `features_rest` parameter per sub-model (background F = 1, objects
// F = fourier_features_dim); the fused front end above still wanted ONE [N,F,3] / [N,K-1,3] tensor, i.e. the caller's
// `torch.cat` (180 MB read + 180 MB write per step at 1 M Gaussians for features_rest, a zero-padded copy for
// features_dc) and autograd's split of the gradient on the way back.  Here the kernel takes the sub-models as they are:
// a by-value table of up to 32 parts (rows, first row in the aggregated order, pointers, Fourier dimension), the grid is
// the concatenation of the parts' own spans of 64 rows (a wave never straddles two parts), the part index IS the object
// index (pose row / idft row), and the backward writes each part's gradients into that part's own tensors.
constexpr int SH_MAX_PARTS = 32;
struct ShParts {
    int n_parts;
    int span0[SH_MAX_PARTS + 1];        // first 64-row span of part p in the grid; span0[n_parts] = total spans
    int row0[SH_MAX_PARTS];             // first row of part p in the aggregated (means / colours) order
    int rows[SH_MAX_PARTS];
    int F[SH_MAX_PARTS];
    const float *dc[SH_MAX_PARTS];      // [rows, F, 3]
    const float *rest[SH_MAX_PARTS];    // [rows, K-1, 3]
    float *v_dc[SH_MAX_PARTS];
    float *v_rest[SH_MAX_PARTS];
};

// the part `p` that grid span `span` belongs to, the span's first row INSIDE that part and its row count (0 rows
// behind the last span)
__device__ __forceinline__ void sh_part_span(const ShParts &P, int span, int &p, int &r0, int &cnt) {
    const bool live = span < P.span0[P.n_parts];
    p = 0;
    if (live)
        while (p + 1 < P.n_parts && span >= P.span0[p + 1]) ++p;
    r0 = live ? (span - P.span0[p]) * 64 : 0;
    cnt = live ? max(0, min(64, P.rows[p] - r0)) : 0;
}
// view direction of aggregated row i, a row of part (= object) p
__device__ __forceinline__ int sh_part_bases(int i, int p, const float *__restrict__ means,
                                             const float *__restrict__ cam_pos, const float *__restrict__ poses,
                                             int deg, float *b) {
    float m0 = means[3 * i], m1 = means[3 * i + 1], m2 = means[3 * i + 2];
    if (poses != nullptr) pose_apply(poses + 16 * (size_t)p, m0, m1, m2);
    return sh_bases(m0 - cam_pos[0], m1 - cam_pos[1], m2 - cam_pos[2], deg, b);
}

template <int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sh_fwd_parts_kernel(
    ShParts P, int deg, const float *__restrict__ means, const float *__restrict__ cam_pos,
    const float *__restrict__ idft, int idft_stride, const float *__restrict__ poses, int post,
    float *__restrict__ colors) {
    constexpr int KC = (K - 1) * 3, LS = (KC | 1);
    __shared__ float lds[WAVES][64 * (KC > 0 ? LS : 1)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int p, r0, cnt;
    sh_part_span(P, blockIdx.x * WAVES + wave, p, r0, cnt);
    float *my = lds[wave];
    if constexpr (KC > 0) stage_rows<KC, LS>(my, P.rest[p] + (size_t)r0 * KC, cnt, lane);
    __syncthreads();
    if (lane >= cnt) return;
    const int r = r0 + lane, i = P.row0[p] + r;
    float b[25];
    const int nb = sh_part_bases(i, p, means, cam_pos, poses, deg, b);
    const int F = P.F[p];
    float d0, d1, d2;
    sh_dc_eff(P.dc[p] + (size_t)r * F * 3, F, idft + (size_t)p * idft_stride, d0, d1, d2);
    float a0 = b[0] * d0, a1 = b[0] * d1, a2 = b[0] * d2;
    sh_eval_bands<1, K>(b, nb, my + lane * LS, a0, a1, a2);
    if (post) sh_post(a0, a1, a2);
    colors[3 * i] = a0; colors[3 * i + 1] = a1; colors[3 * i + 2] = a2;
}

template <int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sh_bwd_parts_kernel(
    ShParts P, int deg, const float *__restrict__ means, const float *__restrict__ cam_pos,
    const float *__restrict__ idft, int idft_stride, const float *__restrict__ poses, int post,
    const float *__restrict__ colors, const float *__restrict__ v_colors) {
    constexpr int KC = (K - 1) * 3, LS = (KC | 1);
    __shared__ float lds[WAVES][64 * (KC > 0 ? LS : 1)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int p, r0, cnt;
    sh_part_span(P, blockIdx.x * WAVES + wave, p, r0, cnt);
    float *my = lds[wave];
    if (lane < cnt) {
        const int r = r0 + lane, i = P.row0[p] + r;
        float b[25];
        const int nb = sh_part_bases(i, p, means, cam_pos, poses, deg, b);
        float v0 = v_colors[3 * i], v1 = v_colors[3 * i + 1], v2 = v_colors[3 * i + 2];
        if (post) sh_post_gate(colors + 3 * i, v0, v1, v2);
        const int F = P.F[p];
        sh_dc_fan_out(P.v_dc[p] + (size_t)r * F * 3, F, idft + (size_t)p * idft_stride, b[0], v0, v1, v2);
        sh_fill_row<1, K>(my + lane * LS, b, nb, v0, v1, v2);
    }
    __syncthreads();
    if constexpr (KC > 0) {
        if (cnt > 0) drain_rows<KC, LS, 0, false>(P.v_rest[p] + (size_t)r0 * KC, my, cnt, lane);
    }
}

// ---- multi-view SH backward for data-parallel training ---------------------------------
// v_coeffs[n,k,c] = sum_r basis_k(dir_{r,n}) * v_colors[r,n,c]: the SH gradient of ONE view is a rank-1 outer
// product (K bases x 3 channels) of two things that are tiny on the wire — the 3-float colour gradient and the
// view direction (or just the camera position).  Instead of all-reducing the dense [N,K,3] gradient
// (192 B/Gaussian, 2*(R-1)/R of it over xGMI), ranks all-gather v_colors (+ viewdirs or cam_pos) and every rank
// rebuilds the summed gradient locally with this kernel: 4x (cam_pos) or 2x (viewdirs) less traffic on the
// point-to-point links, and the extra compute is hidden behind the 192 B/Gaussian store this kernel does anyway.
template <int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sh_bwd_multi_kernel(
    int n, int deg, int n_views, const float *__restrict__ dirs_all /*[R,n,3] or null*/,
    const float *__restrict__ means /*[n,3] or null*/, const float *__restrict__ cam_pos /*[R,3] or null*/,
    const int32_t *__restrict__ object_ids, const float *__restrict__ poses,
    const float *__restrict__ v_colors_all /*[R,n,3]*/, float scale, float *__restrict__ v_coeffs,
    float *__restrict__ v_dc /*null: v_coeffs is [n,K,3]; else v_dc [n,3] takes band 0, v_coeffs [n,K-1,3] the rest*/) {
    constexpr int KC = K * 3, LS = (KC | 1);
    __shared__ float lds[WAVES][64 * LS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (blockIdx.x * WAVES + wave) * 64;
    const int cnt = max(0, min(64, n - g0));
    float *my = lds[wave];
    if (lane < cnt) {
        const int i = g0 + lane;
        float acc[KC];
#pragma unroll
        for (int e = 0; e < KC; ++e) acc[e] = 0.f;
        for (int r = 0; r < n_views; ++r) {
            float dx, dy, dz;
            if (dirs_all != nullptr) {
                const float *d = dirs_all + ((size_t)r * n + i) * 3;
                dx = d[0]; dy = d[1]; dz = d[2];
            } else {
                fused_viewdir(i, means, cam_pos + 3 * r, object_ids, poses, dx, dy, dz);
            }
            float b[25];
            const int nb = sh_bases(dx, dy, dz, deg, b);
            const float *v = v_colors_all + ((size_t)r * n + i) * 3;
            sh_accumulate<K>(acc, b, nb, v[0], v[1], v[2]);
        }
        float *row = my + lane * LS;
#pragma unroll
        for (int e = 0; e < KC; ++e) row[e] = acc[e] * scale;
    }
    __syncthreads();
    if (v_dc == nullptr) drain_rows<KC, LS, 0, false>(v_coeffs + (size_t)g0 * KC, my, cnt, lane);
    else drain_dc_rest<KC, LS>(v_dc, v_coeffs, g0, my, cnt, lane);
}

// ---- batched views (include/sgn_rast.h "Batched views") -----------------------------------------------------------------
// The fused SH front end for B cameras at once: a wave stages its 64 rows of features_rest into LDS ONCE and every lane
// evaluates its Gaussian from each camera of the table, colour row b * n + i.  Per view the arithmetic is
// sh_fwd_fused_kernel's with n_fourier = 1 and idft = {1} (dc_eff = 0 + dc * 1), operation by operation.  The backward
// sums the views' coefficient gradients in registers in ascending view order (as sh_bwd_multi_kernel, plus the
// clamp's mask of the fused backward) and writes each coefficient once: no atomics.
template <int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sh_views_fwd_kernel(int n, int deg, const SgnViews views,
                                                                  const float *__restrict__ means,
                                                                  const float *__restrict__ dc,
                                                                  const float *__restrict__ rest, int post,
                                                                  float *__restrict__ colors) {
    constexpr int KC = (K - 1) * 3, LS = (KC | 1);
    __shared__ float lds[WAVES][64 * (KC > 0 ? LS : 1)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (blockIdx.x * WAVES + wave) * 64;
    const int cnt = max(0, min(64, n - g0));
    float *my = lds[wave];
    if constexpr (KC > 0) stage_rows<KC, LS>(my, rest + (size_t)g0 * KC, cnt, lane);
    __syncthreads();
    if (lane >= cnt) return;
    const int i = g0 + lane;
    const float m0 = means[3 * i], m1 = means[3 * i + 1], m2 = means[3 * i + 2];
    float d0, d1, d2;
    sh_dc_eff(dc + 3 * i, 1, ShUnitWeight{}, d0, d1, d2);
    for (int v = 0; v < views.n; ++v) {
        float b[25];
        const int nb = sh_bases(m0 - views.pos[v][0], m1 - views.pos[v][1], m2 - views.pos[v][2], deg, b);
        float a0 = b[0] * d0, a1 = b[0] * d1, a2 = b[0] * d2;
        sh_eval_bands<1, K>(b, nb, my + lane * LS, a0, a1, a2);
        if (post) sh_post(a0, a1, a2);
        const size_t o = (size_t)v * n + i;
        colors[3 * o] = a0; colors[3 * o + 1] = a1; colors[3 * o + 2] = a2;
    }
}

template <int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void sh_views_bwd_kernel(int n, int deg, const SgnViews views,
                                                                  const float *__restrict__ means, int post,
                                                                  const float *__restrict__ colors,
                                                                  const float *__restrict__ v_colors,
                                                                  float *__restrict__ v_dc, float *__restrict__ v_rest) {
    constexpr int KC = K * 3, LS = (KC | 1);
    __shared__ float lds[WAVES][64 * LS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g0 = (blockIdx.x * WAVES + wave) * 64;
    const int cnt = max(0, min(64, n - g0));
    float *my = lds[wave];
    if (lane < cnt) {
        const int i = g0 + lane;
        const float m0 = means[3 * i], m1 = means[3 * i + 1], m2 = means[3 * i + 2];
        float acc[KC];
#pragma unroll
        for (int e = 0; e < KC; ++e) acc[e] = 0.f;
        for (int v = 0; v < views.n; ++v) {
            const size_t o = (size_t)v * n + i;
            float v0 = v_colors[3 * o], v1 = v_colors[3 * o + 1], v2 = v_colors[3 * o + 2];
            if (post) sh_post_gate(colors + 3 * o, v0, v1, v2);
            float b[25];
            const int nb = sh_bases(m0 - views.pos[v][0], m1 - views.pos[v][1], m2 - views.pos[v][2], deg, b);
            sh_accumulate<K>(acc, b, nb, v0, v1, v2);
        }
        float *row = my + lane * LS;
#pragma unroll
        for (int e = 0; e < KC; ++e) row[e] = acc[e];
    }
    __syncthreads();
    drain_dc_rest<KC, LS>(v_dc, v_rest, g0, my, cnt, lane);
}

// ---- host side: what every SH entry point shares --------------------------------------------------------------------
// The one rule for (k, degree): degree in 0..4, k a full set of bands, and the bands of `degree` within k.  A zero
// code, or the code and the text of the first condition that fails.
struct ShArgFault {
    int code;
    const char *what;
};
ShArgFault sh_k_degree_fault(int k, int degree) {
    if (!(degree >= 0 && degree <= 4)) return {-2, "degree >= 0 && degree <= 4"};
    if (!(k == 1 || k == 4 || k == 9 || k == 16 || k == 25)) return {-3, "k == 1 || k == 4 || k == 9 || k == 16 || k == 25"};
    if (!((degree + 1) * (degree + 1) <= k)) return {-4, "(degree + 1) * (degree + 1) <= k"};
    return {0, nullptr};
}
// ... as three SGN_ARG_CHECKs on the entry's `k` and `degree`
#define SH_CHECK_K_DEGREE()                                                             \
    do {                                                                                \
        const ShArgFault f_ = sh_k_degree_fault(k, degree);                             \
        if (f_.code) {                                                                  \
            sgn_set_error("%s: argument check failed: %s", __func__, f_.what);          \
            return f_.code;                                                             \
        }                                                                               \
    } while (0)

constexpr int sh_waves(int K) { return K > 16 ? 2 : 4; }   // waves per block: keeps static LDS under 64 KiB

// Runtime k (checked) -> compile-time K: calls fn(std::integral_constant<int, K>{}).
template <class Fn>
void sh_dispatch(int k, Fn &&fn) {
    switch (k) {
        case 1: fn(std::integral_constant<int, 1>{}); break;
        case 4: fn(std::integral_constant<int, 4>{}); break;
        case 9: fn(std::integral_constant<int, 9>{}); break;
        case 16: fn(std::integral_constant<int, 16>{}); break;
        default: fn(std::integral_constant<int, 25>{}); break;
    }
}
// One launch of KERNEL<K, WAVES> for the entry's checked `k`: a wave per span of 64 rows, WAVES spans per block.
#define SH_LAUNCH(KERNEL, spans, stream, ...)                                                                  \
    sh_dispatch(k, [&](auto kc_) {                                                                             \
        constexpr int K_ = decltype(kc_)::value, W_ = sh_waves(K_);                                            \
        hipLaunchKernelGGL((KERNEL<K_, W_>), dim3(sgn_cdiv((spans), W_)), dim3(W_ * 64), 0, (stream), __VA_ARGS__); \
    })

}  // namespace

SGN_EXPORT int sgn_sh_fwd(int n, int k, int degree, const float *viewdirs, const float *coeffs,
                          float *colors, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    SH_CHECK_K_DEGREE();
    if (n == 0) return 0;
    SGN_ARG_CHECK(viewdirs && coeffs && colors, -5);
    hipStream_t s = (hipStream_t)stream;
    sgn_timing_begin(SGN_T_SH_FWD, s);
    sh_dispatch(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value, WAVES = sh_waves(K);
        // grid-stride over spans: enough workgroups to fill the LDS-limited residency (160 KB / slab bytes per CU) twice
        const int full = sgn_cdiv(n, WAVES * 64);
        // (tests/sh_fp64.py GRID_CAP and test_gpu_sh_fp64.py's grid-stride cases are sized by this cap)
        const int grid = full < 256 * 6 ? full : 256 * 6;
        hipLaunchKernelGGL((sh_fwd_kernel<K, WAVES>), dim3(grid), dim3(WAVES * 64), 0, s, n, degree, viewdirs, coeffs,
                           colors);
    });
    sgn_timing_end(SGN_T_SH_FWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_sh_bwd(int n, int k, int degree, const float *viewdirs, const float *v_colors,
                          float *v_coeffs, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    SH_CHECK_K_DEGREE();
    if (n == 0) return 0;
    SGN_ARG_CHECK(viewdirs && v_colors && v_coeffs, -5);
    hipStream_t s = (hipStream_t)stream;
    sgn_timing_begin(SGN_T_SH_BWD, s);
    SH_LAUNCH(sh_bwd_kernel, sgn_cdiv(n, 64), s, n, degree, viewdirs, v_colors, v_coeffs);
    sgn_timing_end(SGN_T_SH_BWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_sh_fwd_fused(int n, int k, int degree, const float *means, const float *cam_pos3,
                                const float *features_dc, int n_fourier, const float *features_rest,
                                const int32_t *object_ids, const float *idft, const float *poses, int post_half_clamp,
                                float *colors, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    SH_CHECK_K_DEGREE();
    SGN_ARG_CHECK(n_fourier >= 1 && n_fourier <= 16, -5);
    if (n == 0) return 0;
    SGN_ARG_CHECK(means && cam_pos3 && features_dc && idft && colors && (k == 1 || features_rest), -6);
    hipStream_t s = (hipStream_t)stream;
    sgn_timing_begin(SGN_T_SH_FWD, s);
    SH_LAUNCH(sh_fwd_fused_kernel, sgn_cdiv(n, 64), s, n, degree, means, cam_pos3, features_dc, n_fourier,
              features_rest, object_ids, idft, poses, post_half_clamp, colors);
    sgn_timing_end(SGN_T_SH_FWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_sh_bwd_fused(int n, int k, int degree, const float *means, const float *cam_pos3, int n_fourier,
                                const int32_t *object_ids, const float *idft, const float *poses, int post_half_clamp,
                                const float *colors, const float *v_colors, float *v_features_dc,
                                float *v_features_rest, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0, -1);
    SH_CHECK_K_DEGREE();
    SGN_ARG_CHECK(n_fourier >= 1 && n_fourier <= 16, -5);
    if (n == 0) return 0;
    SGN_ARG_CHECK(means && cam_pos3 && idft && colors && v_colors && v_features_dc && (k == 1 || v_features_rest), -6);
    hipStream_t s = (hipStream_t)stream;
    sgn_timing_begin(SGN_T_SH_BWD, s);
    SH_LAUNCH(sh_bwd_fused_kernel, sgn_cdiv(n, 64), s, n, degree, means, cam_pos3, n_fourier, object_ids, idft,
              poses, post_half_clamp, colors, v_colors, v_features_dc, v_features_rest);
    sgn_timing_end(SGN_T_SH_BWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_sh_bwd_multi(int n, int k, int degree, int n_views, const float *viewdirs_all, const float *means,
                                const float *cam_pos_all, const int32_t *object_ids, const float *poses,
                                const float *v_colors_all, float scale, float *v_coeffs, float *v_dc,
                                sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 0 && n_views >= 1, -1);
    SH_CHECK_K_DEGREE();
    if (n == 0) return 0;
    SGN_ARG_CHECK(v_colors_all && (v_coeffs || (v_dc && k == 1)), -5);
    SGN_ARG_CHECK((viewdirs_all != nullptr) != (means != nullptr && cam_pos_all != nullptr), -6);
    hipStream_t s = (hipStream_t)stream;
    sgn_timing_begin(SGN_T_SH_BWD, s);
    SH_LAUNCH(sh_bwd_multi_kernel, sgn_cdiv(n, 64), s, n, degree, n_views, viewdirs_all, means, cam_pos_all,
              object_ids, poses, v_colors_all, scale, v_coeffs, v_dc);
    sgn_timing_end(SGN_T_SH_BWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

// ---- Fourier DC fan-out (drop-in graph proofs over the scene graph's aggregation) -------------------------------------
// The scene graph builds an object's effective DC term as `sum(features_dc * idft[..., None], dim=1, keepdim=True)`
// (sgn_splatfacto_scene_graph.py:239-247) and concatenates those per-object terms (:356).  When the SH node's backward
// holds the gradient of the concatenated effective term, v_dc_eff [N,3], each Fourier leaf's gradient is
// v_features_dc[r, f, :] = v_dc_eff[row0 + r, :] * idft[f]: one launch for all the objects instead of three autograd
// nodes and two kernels per object.
namespace {
constexpr int FOURIER_MAX_PARTS = 32;
struct FourierParts {
    int n_parts;
    int cum[FOURIER_MAX_PARTS + 1];   // cumulative row counts of the listed parts
    int row0[FOURIER_MAX_PARTS];      // first row of the part in v_dc_eff
    int F[FOURIER_MAX_PARTS];
    const float *w[FOURIER_MAX_PARTS];
    float *out[FOURIER_MAX_PARTS];
};

__global__ __launch_bounds__(256) void fourier_dc_bwd_kernel(FourierParts P, const float *__restrict__ v_dc_eff) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P.cum[P.n_parts]) return;
    int p = 0;
    while (p + 1 < P.n_parts && t >= P.cum[p + 1]) ++p;
    const int r = t - P.cum[p];
    const size_t row = (size_t)P.row0[p] + r;
    const float v0 = v_dc_eff[3 * row], v1 = v_dc_eff[3 * row + 1], v2 = v_dc_eff[3 * row + 2];
    const int F = P.F[p];
    float *o = P.out[p] + (size_t)r * F * 3;
    const float *w = P.w[p];
    for (int f = 0; f < F; ++f) {
        const float wf = w[f];
        o[3 * f] = v0 * wf; o[3 * f + 1] = v1 * wf; o[3 * f + 2] = v2 * wf;
    }
}
}  // namespace

SGN_EXPORT int sgn_fourier_dc_bwd(int n_parts, const int32_t *row0_host, const int32_t *rows_host,
                                  const int32_t *n_fourier_host, const float *const *weights_host,
                                  float *const *out_host, const float *v_dc_eff, sgn_stream_t stream) {
    SGN_ARG_CHECK(n_parts >= 0, -1);
    if (n_parts == 0) return 0;
    SGN_ARG_CHECK(row0_host && rows_host && n_fourier_host && weights_host && out_host && v_dc_eff, -2);
    for (int base = 0; base < n_parts; base += FOURIER_MAX_PARTS) {
        FourierParts P;
        P.n_parts = n_parts - base < FOURIER_MAX_PARTS ? n_parts - base : FOURIER_MAX_PARTS;
        P.cum[0] = 0;
        for (int i = 0; i < P.n_parts; ++i) {
            SGN_ARG_CHECK(rows_host[base + i] >= 0 && row0_host[base + i] >= 0, -3);
            SGN_ARG_CHECK(n_fourier_host[base + i] >= 1 && n_fourier_host[base + i] <= 64, -4);
            SGN_ARG_CHECK(weights_host[base + i] && out_host[base + i], -5);
            P.cum[i + 1] = P.cum[i] + rows_host[base + i];
            P.row0[i] = row0_host[base + i];
            P.F[i] = n_fourier_host[base + i];
            P.w[i] = weights_host[base + i];
            P.out[i] = out_host[base + i];
        }
        if (P.cum[P.n_parts] == 0) continue;
        hipLaunchKernelGGL(fourier_dc_bwd_kernel, dim3(sgn_cdiv(P.cum[P.n_parts], 256)), dim3(256), 0,
                           (hipStream_t)stream, P, v_dc_eff);
    }
    SGN_LAUNCH_CHECK();
    return 0;
}

// ---- fused SH over un-concatenated sub-models: entry points
namespace {
int fill_parts(ShParts &P, int n_parts, const int32_t *rows_host, const int32_t *n_fourier_host,
               const float *const *dc_host, const float *const *rest_host, float *const *v_dc_host,
               float *const *v_rest_host, int k, bool backward) {
    if (n_parts < 1 || n_parts > SH_MAX_PARTS || !rows_host || !n_fourier_host) return -1;
    if (backward ? !v_dc_host : !dc_host) return -1;
    P.n_parts = n_parts;
    int span = 0, row = 0;
    for (int p = 0; p < n_parts; ++p) {
        if (rows_host[p] < 0 || n_fourier_host[p] < 1 || n_fourier_host[p] > 16) return -2;
        P.span0[p] = span; P.row0[p] = row; P.rows[p] = rows_host[p]; P.F[p] = n_fourier_host[p];
        P.dc[p] = backward ? nullptr : dc_host[p];
        P.rest[p] = (backward || k == 1) ? nullptr : rest_host[p];
        P.v_dc[p] = backward ? v_dc_host[p] : nullptr;
        P.v_rest[p] = (backward && k > 1) ? v_rest_host[p] : nullptr;
        if (rows_host[p] > 0) {
            if (!backward && (!dc_host[p] || (k > 1 && !rest_host[p]))) return -3;
            if (backward && (!v_dc_host[p] || (k > 1 && !v_rest_host[p]))) return -3;
        }
        span += (rows_host[p] + 63) / 64;
        row += rows_host[p];
    }
    P.span0[n_parts] = span;
    for (int p = n_parts; p < SH_MAX_PARTS; ++p) { P.row0[p] = 0; P.rows[p] = 0; P.F[p] = 1; P.dc[p] = P.rest[p] = nullptr; P.v_dc[p] = P.v_rest[p] = nullptr; }
    for (int p = n_parts + 1; p <= SH_MAX_PARTS; ++p) P.span0[p] = span;
    return span;
}
}  // namespace

SGN_EXPORT int sgn_sh_fwd_parts(int n_parts, const int32_t *rows_host, const int32_t *n_fourier_host,
                                const float *const *features_dc_host, const float *const *features_rest_host, int k,
                                int degree, const float *means, const float *cam_pos3, const float *idft,
                                int idft_stride, const float *poses, int post_half_clamp, float *colors,
                                sgn_stream_t stream) {
    SH_CHECK_K_DEGREE();
    SGN_ARG_CHECK(means && cam_pos3 && idft && colors && idft_stride >= 1 && (k == 1 || features_rest_host), -6);
    ShParts P;
    const int spans = fill_parts(P, n_parts, rows_host, n_fourier_host, features_dc_host, features_rest_host, nullptr, nullptr,
                                 k, false);
    SGN_ARG_CHECK(spans >= 0, -7);
    if (spans == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    sgn_timing_begin(SGN_T_SH_FWD, s);
    SH_LAUNCH(sh_fwd_parts_kernel, spans, s, P, degree, means, cam_pos3, idft, idft_stride, poses,
              post_half_clamp, colors);
    sgn_timing_end(SGN_T_SH_FWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_sh_bwd_parts(int n_parts, const int32_t *rows_host, const int32_t *n_fourier_host, int k, int degree,
                                const float *means, const float *cam_pos3, const float *idft, int idft_stride,
                                const float *poses, int post_half_clamp, const float *colors, const float *v_colors,
                                float *const *v_features_dc_host, float *const *v_features_rest_host,
                                sgn_stream_t stream) {
    SH_CHECK_K_DEGREE();
    SGN_ARG_CHECK(means && cam_pos3 && idft && colors && v_colors && v_features_dc_host && idft_stride >= 1 &&
                      (k == 1 || v_features_rest_host), -6);
    ShParts P;
    const int spans = fill_parts(P, n_parts, rows_host, n_fourier_host, nullptr, nullptr, v_features_dc_host,
                                 v_features_rest_host, k, true);
    SGN_ARG_CHECK(spans >= 0, -7);
    if (spans == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    sgn_timing_begin(SGN_T_SH_BWD, s);
    SH_LAUNCH(sh_bwd_parts_kernel, spans, s, P, degree, means, cam_pos3, idft, idft_stride, poses,
              post_half_clamp, colors, v_colors);
    sgn_timing_end(SGN_T_SH_BWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

// ---- batched views: entry points
namespace {
int sh_views(const char *fn, bool fwd, int n_views, int n, int k, int degree, const sgn_view_cam *cams,
             const float *means, const float *dc, const float *rest, int post, const float *colors,
             const float *v_colors, float *out_colors, float *v_dc, float *v_rest, hipStream_t s) {
    if (n_views < 1 || n_views > SGN_VIEWS_MAX) {
        sgn_set_error("%s: n_views %d outside [1, %d]", fn, n_views, SGN_VIEWS_MAX);
        return -1;
    }
    if (!sgn_views_rows_ok(n_views, n)) {
        sgn_set_error("%s: n %d: need n >= 0 and n_views * n < 2^28", fn, n);
        return -2;
    }
    if (sh_k_degree_fault(k, degree).code) {
        sgn_set_error("%s: k %d / degree %d", fn, k, degree);
        return -3;
    }
    if (!cams || (n > 0 && (!means || (fwd ? (!dc || !out_colors || (k > 1 && !rest))
                                           : (!colors || !v_colors || !v_dc || (k > 1 && !v_rest)))))) {
        sgn_set_error("%s: a required pointer is NULL", fn);
        return -4;
    }
    if (n == 0) return 0;
    const SgnViews t = sgn_views_table(n_views, cams, 16, 16, false);
    sgn_timing_begin(fwd ? SGN_T_SH_FWD : SGN_T_SH_BWD, s);
    if (fwd) SH_LAUNCH(sh_views_fwd_kernel, sgn_cdiv(n, 64), s, n, degree, t, means, dc, rest, post, out_colors);
    else SH_LAUNCH(sh_views_bwd_kernel, sgn_cdiv(n, 64), s, n, degree, t, means, post, colors, v_colors, v_dc, v_rest);
    sgn_timing_end(fwd ? SGN_T_SH_FWD : SGN_T_SH_BWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}
}  // namespace

SGN_EXPORT int sgn_sh_views_fwd(int n_views, int n, int k, int degree, const sgn_view_cam *cams, const float *means,
                                const float *features_dc, const float *features_rest, int post_half_clamp,
                                float *colors, sgn_stream_t stream) {
    return sh_views(__func__, true, n_views, n, k, degree, cams, means, features_dc, features_rest, post_half_clamp,
                    nullptr, nullptr, colors, nullptr, nullptr, (hipStream_t)stream);
}

SGN_EXPORT int sgn_sh_views_bwd(int n_views, int n, int k, int degree, const sgn_view_cam *cams, const float *means,
                                int post_half_clamp, const float *colors, const float *v_colors, float *v_features_dc,
                                float *v_features_rest, sgn_stream_t stream) {
    return sh_views(__func__, false, n_views, n, k, degree, cams, means, nullptr, nullptr, post_half_clamp, colors,
                    v_colors, nullptr, v_features_dc, v_features_rest, (hipStream_t)stream);
}
