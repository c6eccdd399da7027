// bilagrid.hip — per-image bilateral-grid colour correction: the fused slice and its backward, gfx950.
//
// THE DEFINITION (include/sgn_rast.h "BILATERAL GRID"; tests/bilagrid_fp64.py restates it in float64).
// A grid is g[L, Hg, Wg, 12], float32, cell-major: the 12 coefficients of a cell are contiguous (48 bytes), coefficient
// 4 r + c is row r, column c of a 3x4 affine, c = 3 the bias; L, Hg, Wg >= 1.  For pixel (i, j) of an H x W image with
// colour p = (R, G, B):
//     gx = (j + 0.5) / W * (Wg - 1)              gy = (i + 0.5) / H * (Hg - 1)
//     luma = 0.299 R + 0.587 G + 0.114 B         gz = clamp(luma, 0, 1) * (L - 1)
// (grid_sample(align_corners=True, padding_mode="border") on (x, y, luma) in [0,1]^3),
//     x0 = floor(gx), x1 = min(x0 + 1, Wg - 1), fx = gx - x0        and the same for y and z,
// A = the trilinear mix of the eight cells taken as NESTED LERPS a + f * (b - a): z innermost, then x, then y, and
//     out_r = A[r,0] R + A[r,1] G + A[r,2] B + A[r,3]               (left to right).
// The lerp form is part of the contract: a + f * (a - a) == a, so a grid of identity affines returns its input bit for
// bit.  Gradients, with w_cell the product of the cell's three lerp weights, dA = A|z1 - A|z0 (the z-differences b - a
// of the innermost lerps, mixed over x and y as A is; exactly zero when z0 == z1) and lw the three luma weights:
//     v_g[cell][4 r + c] += w_cell * v_out_r * (R, G, B, 1)[c]
//     v_p_k = sum_r v_out_r A[r,k] + lw_k * (L - 1) * [0 < luma < 1] * sum_r v_out_r * (dA[r,:] . (R, G, B, 1))
// The guidance term is kept; pixel positions get no gradient.  fp32, no contraction (-ffp-contract=off): every product
// and sum of the forward and of v_p is its own rounding, IEEE division for the two pixel coordinates; v_g's running sums
// are spelled fmaf.
//
// THE FORWARD is a streaming kernel, one pixel per lane: 12 B in, 12 B out, the eight cells read through the cache as
// 24 16-byte loads (a wave usually sits in one xy cell, so they are near-broadcasts; 16 x 16 x 8 cells are 98 KB).
// v_p is its twin: the same loads give A and dA, one plain store per pixel.
//
// v_g, the design that was built: a GATHER with the sums PRIVATISED IN REGISTERS, a cross-lane reduction per z-level,
// the waves of a workgroup summed through LDS in a fixed order, and only then one shaped global_atomic_add_f32 per
// coefficient.  Why: all 64 lanes of a wave usually share an xy cell, so per-lane atomics — global or LDS — put them on
// one address 96 times per pixel.  The first version of this file did that into LDS boxes replicated 32 times (one
// replica per bank, no two lanes of an instruction on one address): correct, and 1256 us per 1280 x 1920 image at
// 16 x 16 x 8 cells — ds_add_f32 retires about one wave-instruction per 220 cycles per CU whatever the addresses
// (profiles/bilagrid.md).  So the scatter was turned round.  A workgroup owns ONE xy cell (cx, cy) and a band of the
// image rows whose gy lies within one cell of cy; its four waves take the band's rows in turn, lanes stride the columns
// whose gx lies within one cell of cx, and every lane keeps the cell's 12 coefficients for up to 8 z-levels in
// registers: acc[level][4 r + c] = fmaf(w_level * (w_x w_y v_out_r), (R, G, B, 1)[c], acc).  The weights are the
// definition's own — (x0 == cx ? 1 - fx : 0) + (x1 == cx ? fx : 0) — so a pixel outside the cell's support adds an exact
// zero and the band / column ranges only have to be supersets.  A level no lane of the wave touches is skipped (a
// wave-uniform branch: smooth images touch one or two).  Each pixel is read by the four xy cells around it, through the
// cache.  At the end the 12 x levels sums are reduced across the wave's lanes, across the workgroup's waves through LDS
// in wave order, and added to v_g with one atomic each (about 100 per workgroup, 48-byte runs): v_g's last bits depend
// on the order in which the bands of one cell arrive.  The forward and v_p are bit-identical from run to run.
// THE OPPOSITE REGIME — a grid finer than the pixels — is the same code: a cell's band is a few pixels, most lanes idle.
// It only has to be right.  More than 8 z-levels: the gather runs once per 8 levels.
#include <algorithm>

#include "sgn_common.h"

namespace {

constexpr int BG_GATHER_THREADS = 256, BG_GATHER_WAVES = BG_GATHER_THREADS / 64;
constexpr int BG_MAX_LEVELS = 8;                            // z-levels one gather pass keeps in registers

struct BgDims { int L, Hg, Wg, H, W, n_pix; };

struct BgAxis { int i0, i1; float f; };

// cell pair and weight of a grid coordinate g in [0, n - 1] (NaN cannot reach here: the luminance is clamped first)
__device__ __forceinline__ BgAxis bg_axis(float g, int n) {
    BgAxis a;
    a.i0 = min(max((int)floorf(g), 0), n - 1);
    a.i1 = min(a.i0 + 1, n - 1);
    a.f = g - (float)a.i0;
    return a;
}
__device__ __forceinline__ float bg_coord(int k, int size, int cells) {
    return __fdiv_rn((float)k + 0.5f, (float)size) * (float)(cells - 1);
}
__device__ __forceinline__ float bg_luma(float R, float G, float B) { return 0.299f * R + 0.587f * G + 0.114f * B; }
__device__ __forceinline__ float bg_lerp(float a, float b, float f) { return a + f * (b - a); }

// the eight cells of a pixel: offsets in floats, index = zbit + 2 xbit + 4 ybit
__device__ __forceinline__ void bg_cells(const BgDims &d, const BgAxis &z, const BgAxis &x, const BgAxis &y, int (&o)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int zz = (k & 1) ? z.i1 : z.i0, xx = (k & 2) ? x.i1 : x.i0, yy = (k & 4) ? y.i1 : y.i0;
        o[k] = ((zz * d.Hg + yy) * d.Wg + xx) * 12;
    }
}

// row r of A (and of dA) at a pixel: nested lerps, z innermost, then x, then y
template <bool WITH_D>
__device__ __forceinline__ void bg_row(const float *__restrict__ g, const int (&o)[8], int r, float fz, float fx,
                                       float fy, float (&A)[4], float (&D)[4]) {
    float4 c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = *reinterpret_cast<const float4 *>(g + o[k] + 4 * r);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float c0 = (&c[0].x)[q], c1 = (&c[1].x)[q], c2 = (&c[2].x)[q], c3 = (&c[3].x)[q];
        const float c4 = (&c[4].x)[q], c5 = (&c[5].x)[q], c6 = (&c[6].x)[q], c7 = (&c[7].x)[q];
        const float d00 = c1 - c0, d10 = c3 - c2, d01 = c5 - c4, d11 = c7 - c6;
        const float a00 = c0 + fz * d00, a10 = c2 + fz * d10, a01 = c4 + fz * d01, a11 = c6 + fz * d11;
        A[q] = bg_lerp(bg_lerp(a00, a10, fx), bg_lerp(a01, a11, fx), fy);
        if (WITH_D) D[q] = bg_lerp(bg_lerp(d00, d10, fx), bg_lerp(d01, d11, fx), fy);
    }
}

__global__ __launch_bounds__(256) void bilagrid_slice_fwd_kernel(BgDims d, const float *__restrict__ grid,
                                                                 const float *__restrict__ rgb,
                                                                 float *__restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= d.n_pix) return;
    const int i = idx / d.W, j = idx - i * d.W;
    const float R = rgb[3 * idx], G = rgb[3 * idx + 1], B = rgb[3 * idx + 2];
    const BgAxis x = bg_axis(bg_coord(j, d.W, d.Wg), d.Wg), y = bg_axis(bg_coord(i, d.H, d.Hg), d.Hg);
    const BgAxis z = bg_axis(fminf(fmaxf(bg_luma(R, G, B), 0.f), 1.f) * (float)(d.L - 1), d.L);
    int o[8];
    bg_cells(d, z, x, y, o);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float A[4], D[4];
        bg_row<false>(grid, o, r, z.f, x.f, y.f, A, D);
        out[3 * idx + r] = A[0] * R + A[1] * G + A[2] * B + A[3];
    }
}

// v_rgb alone: the forward's twin, one pixel per lane, one plain store per pixel
__global__ __launch_bounds__(256) void bilagrid_slice_bwd_rgb_kernel(BgDims d, const float *__restrict__ grid,
                                                                     const float *__restrict__ rgb,
                                                                     const float *__restrict__ v_out,
                                                                     float *__restrict__ v_rgb) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= d.n_pix) return;
    const int i = idx / d.W, j = idx - i * d.W;
    const float R = rgb[3 * idx], G = rgb[3 * idx + 1], B = rgb[3 * idx + 2];
    const float v[3] = {v_out[3 * idx], v_out[3 * idx + 1], v_out[3 * idx + 2]};
    const BgAxis x = bg_axis(bg_coord(j, d.W, d.Wg), d.Wg), y = bg_axis(bg_coord(i, d.H, d.Hg), d.Hg);
    const float luma = bg_luma(R, G, B);
    const BgAxis z = bg_axis(fminf(fmaxf(luma, 0.f), 1.f) * (float)(d.L - 1), d.L);
    int o[8];
    bg_cells(d, z, x, y, o);
    float s[3] = {0.f, 0.f, 0.f}, guide = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float A[4], D[4];
        bg_row<true>(grid, o, r, z.f, x.f, y.f, A, D);
        const float dot = D[0] * R + D[1] * G + D[2] * B + D[3];
        if (r == 0) {
            s[0] = v[0] * A[0]; s[1] = v[0] * A[1]; s[2] = v[0] * A[2];
            guide = v[0] * dot;
        } else {
            s[0] = s[0] + v[r] * A[0]; s[1] = s[1] + v[r] * A[1]; s[2] = s[2] + v[r] * A[2];
            guide = guide + v[r] * dot;
        }
    }
    if (luma > 0.f && luma < 1.f) {
        const float gl = (float)(d.L - 1) * guide;
        s[0] = s[0] + 0.299f * gl; s[1] = s[1] + 0.587f * gl; s[2] = s[2] + 0.114f * gl;
    }
    v_rgb[3 * idx] = s[0]; v_rgb[3 * idx + 1] = s[1]; v_rgb[3 * idx + 2] = s[2];
}

// the definition's weight of cell c on an axis: both terms when the pair is clamped onto one cell (f is 0 there)
__device__ __forceinline__ float bg_weight(const BgAxis &a, int c) {
    return (a.i0 == c ? 1.f - a.f : 0.f) + (a.i1 == c ? a.f : 0.f);
}
// pixel indices whose coordinate can lie within one cell of c: a superset, [lo, hi) clipped to [0, size)
__device__ __forceinline__ void bg_support(int c, int size, int cells, int &lo, int &hi) {
    lo = 0; hi = size;
    if (cells > 1) {
        const float per = (float)size / (float)(cells - 1);              // pixels per cell
        lo = max(0, (int)floorf((float)(c - 1) * per - 0.5f) - 2);
        hi = min(size, (int)ceilf((float)(c + 1) * per - 0.5f) + 3);
    }
}

// v_grid += the sums of one xy cell over one band of rows_per_wg image rows, levels [level0, level0 + LC).
// blockIdx.x: the cell, cy * Wg + cx; blockIdx.y: the band within the cell's support.
template <int LC>
__global__ __launch_bounds__(BG_GATHER_THREADS) void bilagrid_slice_bwd_grid_kernel(BgDims d, int level0, int rows_per_wg,
                                                                                   const float *__restrict__ rgb,
                                                                                   const float *__restrict__ v_out,
                                                                                   float *__restrict__ v_grid) {
    __shared__ float part[BG_GATHER_WAVES][LC * 12];
    const int cy = blockIdx.x / d.Wg, cx = blockIdx.x - cy * d.Wg;
    const int rows = min(d.H, (d.n_pix + d.W - 1) / d.W);                       // image rows that hold a pixel
    int ilo, ihi, jlo, jhi;
    bg_support(cy, d.H, d.Hg, ilo, ihi);
    bg_support(cx, d.W, d.Wg, jlo, jhi);
    ihi = min(ihi, rows);
    const int r0 = ilo + blockIdx.y * rows_per_wg, r1 = min(ihi, r0 + rows_per_wg);
    if (r0 >= r1) return;                                                        // (the whole workgroup)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[LC][12];
#pragma unroll
    for (int l = 0; l < LC; ++l)
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[l][k] = 0.f;
    for (int i = r0 + wave; i < r1; i += BG_GATHER_WAVES) {
        const float wy = bg_weight(bg_axis(bg_coord(i, d.H, d.Hg), d.Hg), cy);
        for (int j = jlo + lane; j < jhi; j += 64) {
            const int idx = i * d.W + j;
            if (idx >= d.n_pix) break;
            const float wxy = bg_weight(bg_axis(bg_coord(j, d.W, d.Wg), d.Wg), cx) * wy;
            const float R = rgb[3 * idx], G = rgb[3 * idx + 1], B = rgb[3 * idx + 2];
            const float u0 = wxy * v_out[3 * idx], u1 = wxy * v_out[3 * idx + 1], u2 = wxy * v_out[3 * idx + 2];
            const BgAxis z = bg_axis(fminf(fmaxf(bg_luma(R, G, B), 0.f), 1.f) * (float)(d.L - 1), d.L);
#pragma unroll
            for (int l = 0; l < LC; ++l) {
                const float wl = bg_weight(z, level0 + l);
                if (!__any(wl != 0.f)) continue;                                // wave-uniform
                const float t0 = wl * u0, t1 = wl * u1, t2 = wl * u2;
                acc[l][0] = fmaf(t0, R, acc[l][0]); acc[l][1] = fmaf(t0, G, acc[l][1]);
                acc[l][2] = fmaf(t0, B, acc[l][2]); acc[l][3] = acc[l][3] + t0;
                acc[l][4] = fmaf(t1, R, acc[l][4]); acc[l][5] = fmaf(t1, G, acc[l][5]);
                acc[l][6] = fmaf(t1, B, acc[l][6]); acc[l][7] = acc[l][7] + t1;
                acc[l][8] = fmaf(t2, R, acc[l][8]); acc[l][9] = fmaf(t2, G, acc[l][9]);
                acc[l][10] = fmaf(t2, B, acc[l][10]); acc[l][11] = acc[l][11] + t2;
            }
        }
    }
    // across the lanes (every lane is back here: the loops above end per lane, nothing returned), then across the waves
#pragma unroll
    for (int l = 0; l < LC; ++l)
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            float s = acc[l][k];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
            if (lane == 0) part[wave][l * 12 + k] = s;
        }
    __syncthreads();
    const int e = threadIdx.x;
    if (e < LC * 12) {
        float s = part[0][e];
#pragma unroll
        for (int w = 1; w < BG_GATHER_WAVES; ++w) s += part[w][e];
        const int level = level0 + e / 12;
        if (level < d.L && s != 0.f) atomicAdd(v_grid + ((level * d.Hg + cy) * d.Wg + cx) * 12 + (e - (e / 12) * 12), s);
    }
}

}  // namespace

int sgn_bilagrid_slice_fwd_launch(int L, int Hg, int Wg, const float *grid, int H, int W, int n_pix, const float *rgb,
                                  float *out, sgn_stream_t stream) {
    const BgDims d = {L, Hg, Wg, H, W, n_pix};
    hipLaunchKernelGGL(bilagrid_slice_fwd_kernel, dim3(sgn_cdiv(n_pix, 256)), dim3(256), 0, (hipStream_t)stream, d, grid,
                       rgb, out);
    SGN_LAUNCH_CHECK();
    return 0;
}

int sgn_bilagrid_slice_bwd_launch(int L, int Hg, int Wg, const float *grid, int H, int W, int n_pix, const float *rgb,
                                  const float *v_out, float *v_rgb, float *v_grid, sgn_stream_t stream) {
    const BgDims d = {L, Hg, Wg, H, W, n_pix};
    if (v_rgb != nullptr) {
        hipLaunchKernelGGL(bilagrid_slice_bwd_rgb_kernel, dim3(sgn_cdiv(n_pix, 256)), dim3(256), 0, (hipStream_t)stream, d,
                           grid, rgb, v_out, v_rgb);
        SGN_LAUNCH_CHECK();
    }
    if (v_grid == nullptr) return 0;
    // bands: the rows of a cell's support (a superset, as bg_support counts them) cut so that ~2048 workgroups exist
    const int rows = (int)std::min<int64_t>(H, sgn_cdiv(n_pix, W));
    const int support = Hg > 1 ? (int)std::min<int64_t>(rows, 2 * (int64_t)sgn_cdiv(H, Hg - 1) + 8) : rows;
    const int64_t cells = (int64_t)Hg * Wg;
    const int rows_per_wg = (int)std::min<int64_t>(64, std::max<int64_t>(BG_GATHER_WAVES, cells * support / 2048));
    const dim3 blocks((unsigned)cells, (unsigned)sgn_cdiv(support, rows_per_wg));
    for (int level0 = 0; level0 < L; level0 += BG_MAX_LEVELS) {
        const int left = L - level0;
        if (left == 1)
            hipLaunchKernelGGL(bilagrid_slice_bwd_grid_kernel<1>, blocks, dim3(BG_GATHER_THREADS), 0, (hipStream_t)stream, d,
                               level0, rows_per_wg, rgb, v_out, v_grid);
        else if (left <= 4)
            hipLaunchKernelGGL(bilagrid_slice_bwd_grid_kernel<4>, blocks, dim3(BG_GATHER_THREADS), 0, (hipStream_t)stream, d,
                               level0, rows_per_wg, rgb, v_out, v_grid);
        else
            hipLaunchKernelGGL(bilagrid_slice_bwd_grid_kernel<BG_MAX_LEVELS>, blocks, dim3(BG_GATHER_THREADS), 0,
                               (hipStream_t)stream, d, level0, rows_per_wg, rgb, v_out, v_grid);
        SGN_LAUNCH_CHECK();
    }
    return 0;
}
