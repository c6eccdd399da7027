// lidar_depth.hip — LiDAR depth supervision: sweeps splatted to a per-pixel target, the fused depth loss with its
// gradient, and the evaluation depth metrics, gfx950.
//
// The reference trains its depth term against depth images made offline, point by point on the CPU
// (data_utils.get_depth_image_from_path loads them).  Here the target is made on the device from the sweeps themselves:
//   begin   depth [H,W] = +inf;
//   splat   one lane per point: the seeding contract's projection (include/sgn_rast.h "LiDAR SEEDING"), then one
//           atomicMin on the uint32 view of the pixel with the bits of pc.z — positive floats order as unsigned
//           integers, so the nearest return wins whatever the arrival order: bit-identical from run to run;
//   finish  one workgroup per 16x16 output tile, the tile and its halo in LDS: a return survives when no return in its
//           (2 radius + 1)^2 window is nearer by more than rel_tol (the LiDAR sits above the camera and sees background
//           between foreground returns); 0 marks a pixel without a return.
// The loss runs one thread per pixel over the pair features.expected_depth renders: D = dsum / alpha against the target,
// L1 or inverse-depth L1, mean over the counted pixels.  The sum and the count are reduced as csrc/semantic_loss.hip
// does — fp32 per-pixel terms into an fp64 sum — per wave with shuffles, across the block's waves through LDS, then one
// fp64 and one integer atomic per block; a one-thread launch forms the mean.  No host read-back: the backward reads the
// count and the incoming gradient from device memory.  The metrics kernel reduces the same way; the block that draws
// the last ticket forms the five figures, so it is one launch.
// The arithmetic is a contract (include/sgn_rast.h "LiDAR DEPTH"): fp32, IEEE division, no contraction.
#include "sgn_common.h"

namespace {

constexpr int LD_BLOCK = 256;
constexpr int LD_WAVES = LD_BLOCK / 64;
constexpr int LD_TILE = 16;
constexpr int LD_MAX_RADIUS = SGN_LIDAR_DEPTH_MAX_RADIUS;
constexpr int LD_HALO = LD_TILE + 2 * LD_MAX_RADIUS;    // 32
constexpr uint32_t INF_BITS = 0x7f800000u;

struct SplatArgs { float L[12]; float V[12]; float fx, fy, cx, cy, min_z, max_depth; int W, H; };

struct LossSums {
    double sum;            // sum of the counted pixels' terms
    unsigned int count;    // counted pixels
    unsigned int pad;
};
static_assert(sizeof(LossSums) == 16, "workspace layout");

struct MetricSums {
    double abs_rel, sq, abs;
    unsigned int count, inlier, ticket, pad;
};
static_assert(sizeof(MetricSums) == 40, "workspace layout");
static_assert(sizeof(MetricSums) <= SGN_DEPTH_LOSS_WS_BYTES, "workspace size");

// M (3x4 row-major) applied to (x, y, z): ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3], as csrc/seed.hip
__device__ __forceinline__ void affine(const float *M, float x, float y, float z, float &ox, float &oy, float &oz) {
    ox = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
    oy = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
    oz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}

__global__ __launch_bounds__(LD_BLOCK) void depth_fill_kernel(int n_pix, uint32_t *__restrict__ depth) {
    const int p = blockIdx.x * LD_BLOCK + threadIdx.x;
    if (p < n_pix) depth[p] = INF_BITS;
}

__global__ __launch_bounds__(LD_BLOCK) void depth_splat_kernel(int n, const float *__restrict__ points, SplatArgs C,
                                                               uint32_t *__restrict__ depth) {
    const int i = blockIdx.x * LD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
    bool live = !(x != x || y != y || z != z) && z > C.min_z;
    float wx, wy, wz, cx_, cy_, cz_;
    affine(C.L, x, y, z, wx, wy, wz);
    live = live && !(fabsf(wx) > 1e5f);
    affine(C.V, wx, wy, wz, cx_, cy_, cz_);
    const float fu = (C.fx * cx_ + C.cx * cz_) / cz_, fv = (C.fy * cy_ + C.cy * cz_) / cz_;
    // trunc(fu) in [0, W) <=> -1 < fu < W (W <= 16384 is exact in fp32); NaN and inf fail a comparison
    const bool vis = cz_ > 0.f && fu > -1.f && fu < (float)C.W && fv > -1.f && fv < (float)C.H;
    if (live && vis && cz_ <= C.max_depth)
        atomicMin(depth + ((size_t)(int)fv * (size_t)C.W + (size_t)(int)fu), __float_as_uint(cz_));
}

// One workgroup per 16x16 output tile.  The minimum over a square window is the minimum over its rows of the minimum
// along each row: two passes of 2 radius + 1 reads through LDS; a minimum is exact, so the order does not matter.
__global__ __launch_bounds__(LD_TILE * LD_TILE) void depth_finish_kernel(int H, int W, int radius, float keep,
                                                                         const float *__restrict__ depth,
                                                                         float *__restrict__ out) {
    __shared__ float tile[LD_HALO][LD_HALO + 1];
    __shared__ float rowmin[LD_HALO][LD_TILE + 1];
    const int tx = threadIdx.x & (LD_TILE - 1), ty = threadIdx.x / LD_TILE;
    const int x0 = blockIdx.x * LD_TILE - radius, y0 = blockIdx.y * LD_TILE - radius;
    const int span = LD_TILE + 2 * radius;
    const float inf = __uint_as_float(INF_BITS);
    for (int k = threadIdx.x; k < span * span; k += LD_TILE * LD_TILE) {
        const int r = k / span, c = k - r * span;
        const int gy = y0 + r, gx = x0 + c;
        tile[r][c] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? depth[(size_t)gy * W + gx] : inf;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < span * LD_TILE; k += LD_TILE * LD_TILE) {
        const int r = k / LD_TILE, c = k - r * LD_TILE;
        float m = inf;
        for (int d = 0; d <= 2 * radius; ++d) m = fminf(m, tile[r][c + d]);
        rowmin[r][c] = m;
    }
    __syncthreads();
    const int gx = blockIdx.x * LD_TILE + tx, gy = blockIdx.y * LD_TILE + ty;
    if (gx >= W || gy >= H) return;
    float m = inf;
    for (int d = 0; d <= 2 * radius; ++d) m = fminf(m, rowmin[ty + d][tx]);
    const float z = tile[ty + radius][tx + radius];
    out[(size_t)gy * W + gx] = (z < inf && z * keep <= m) ? z : 0.f;
}

// counted = z > 0 & alpha > 1e-3 & dsum > 0 & (no mask | mask byte != 0); a NaN fails its comparison
__device__ __forceinline__ bool dl_counted(int p, const float *__restrict__ dsum, const float *__restrict__ alpha,
                                           const float *__restrict__ target, const unsigned char *__restrict__ mask,
                                           float &s, float &a, float &z) {
    s = dsum[p]; a = alpha[p]; z = target[p];
    return z > 0.f && a > 1e-3f && s > 0.f && (mask == nullptr || mask[p] != 0);
}

// residual of one counted pixel: D - z (kind 0) or 1/D - 1/z (kind 1), D = dsum / alpha
__device__ __forceinline__ float dl_residual(int kind, float D, float z) {
    return kind == SGN_DEPTH_LOSS_L1 ? D - z : __fdiv_rn(1.f, D) - __fdiv_rn(1.f, z);
}

// sums over the block: per wave with shuffles, across the waves through LDS; the result is valid in thread 0
template <int N>
__device__ __forceinline__ void block_sums(double (&d)[N], unsigned int (&u)[2]) {
    __shared__ double sd[LD_WAVES][N];
    __shared__ unsigned int su[LD_WAVES][2];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) d[k] += __shfl_xor(d[k], o, 64);
        u[0] += __shfl_xor(u[0], o, 64);
        u[1] += __shfl_xor(u[1], o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sd[wave][k] = d[k];
        su[wave][0] = u[0]; su[wave][1] = u[1];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < LD_WAVES; ++w) {
#pragma unroll
            for (int k = 0; k < N; ++k) d[k] += sd[w][k];
            u[0] += su[w][0]; u[1] += su[w][1];
        }
    }
}

__global__ __launch_bounds__(LD_BLOCK) void depth_loss_fwd_kernel(int n_pix, int kind, const float *__restrict__ dsum,
                                                                  const float *__restrict__ alpha,
                                                                  const float *__restrict__ target,
                                                                  const unsigned char *__restrict__ mask,
                                                                  LossSums *__restrict__ sums) {
    const int p = blockIdx.x * LD_BLOCK + threadIdx.x;
    double d[1] = {0.0};
    unsigned int u[2] = {0u, 0u};
    float s, a, z;
    if (p < n_pix && dl_counted(p, dsum, alpha, target, mask, s, a, z)) {
        d[0] = (double)fabsf(dl_residual(kind, __fdiv_rn(s, a), z));
        u[0] = 1u;
    }
    block_sums<1>(d, u);
    if (threadIdx.x == 0 && u[0] != 0u) {
        atomicAdd(&sums->sum, d[0]);
        atomicAdd(&sums->count, u[0]);
    }
}

__global__ void depth_loss_mean_kernel(const LossSums *__restrict__ sums, float *__restrict__ loss_out,
                                       int32_t *__restrict__ count_out) {
    // an image with no counted pixel: loss 0 (and, in the backward, zero gradients), not 0 / 0
    const unsigned int c = sums->count;
    loss_out[0] = (float)(sums->sum / (double)(c != 0u ? c : 1u));
    count_out[0] = (int32_t)c;
}

__global__ __launch_bounds__(LD_BLOCK) void depth_loss_bwd_kernel(int n_pix, int kind, const float *__restrict__ dsum,
                                                                  const float *__restrict__ alpha,
                                                                  const float *__restrict__ target,
                                                                  const unsigned char *__restrict__ mask,
                                                                  const float *__restrict__ v_loss,
                                                                  const int32_t *__restrict__ count,
                                                                  float *__restrict__ v_dsum,
                                                                  float *__restrict__ v_alpha) {
    const int p = blockIdx.x * LD_BLOCK + threadIdx.x;
    if (p >= n_pix) return;
    float s, a, z, vd = 0.f, va = 0.f;
    if (dl_counted(p, dsum, alpha, target, mask, s, a, z)) {
        const int32_t c = count[0];
        const float g = __fdiv_rn(v_loss[0], (float)(c > 1 ? c : 1));
        const float D = __fdiv_rn(s, a);
        const float r = dl_residual(kind, D, z);
        if (r != 0.f) {                                 // sign 0 at equality: exact zeros
            const float gs = r > 0.f ? g : -g;
            vd = kind == SGN_DEPTH_LOSS_L1 ? __fdiv_rn(gs, a) : __fdiv_rn(__fdiv_rn(-gs, D * D), a);
            va = -vd * D;
        }
    }
    v_dsum[p] = vd;
    v_alpha[p] = va;
}

__global__ __launch_bounds__(LD_BLOCK) void depth_metrics_kernel(int n_pix, const float *__restrict__ dsum,
                                                                 const float *__restrict__ alpha,
                                                                 const float *__restrict__ target,
                                                                 const unsigned char *__restrict__ mask,
                                                                 MetricSums *__restrict__ sums, float *__restrict__ out5) {
    const int p = blockIdx.x * LD_BLOCK + threadIdx.x;
    double d[3] = {0.0, 0.0, 0.0};
    unsigned int u[2] = {0u, 0u};
    float s, a, z;
    if (p < n_pix && dl_counted(p, dsum, alpha, target, mask, s, a, z)) {
        const float D = __fdiv_rn(s, a);
        const float e = fabsf(D - z);
        d[0] = (double)__fdiv_rn(e, z);
        d[1] = (double)(e * e);
        d[2] = (double)e;
        u[0] = 1u;
        u[1] = fmaxf(__fdiv_rn(D, z), __fdiv_rn(z, D)) < 1.25f ? 1u : 0u;
    }
    block_sums<3>(d, u);
    if (threadIdx.x != 0) return;
    if (u[0] != 0u) {
        atomicAdd(&sums->abs_rel, d[0]);
        atomicAdd(&sums->sq, d[1]);
        atomicAdd(&sums->abs, d[2]);
        atomicAdd(&sums->count, u[0]);
        atomicAdd(&sums->inlier, u[1]);
    }
    // the block that draws the last ticket sees every block's sums: all of them are device-scope atomics, ordered
    // before the ticket by the fence, and are read back with atomics as well
    __threadfence();
    if (atomicAdd(&sums->ticket, 1u) != gridDim.x - 1) return;
    __threadfence();
    const unsigned int c = atomicAdd(&sums->count, 0u), in = atomicAdd(&sums->inlier, 0u);
    const double n = (double)(c != 0u ? c : 1u);
    out5[0] = (float)(atomicAdd(&sums->abs_rel, 0.0) / n);
    out5[1] = (float)sqrt(atomicAdd(&sums->sq, 0.0) / n);
    out5[2] = (float)(atomicAdd(&sums->abs, 0.0) / n);
    out5[3] = (float)((double)in / n);
    out5[4] = (float)c;
}

}  // namespace

SGN_EXPORT int sgn_lidar_depth_begin(float *depth, int height, int width, sgn_stream_t stream) {
    SGN_ARG_CHECK(width >= 1 && width <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(height >= 1 && height <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(depth != nullptr, -4);
    const int n_pix = height * width;
    hipLaunchKernelGGL(depth_fill_kernel, dim3(sgn_cdiv(n_pix, LD_BLOCK)), dim3(LD_BLOCK), 0, (hipStream_t)stream, n_pix,
                       (uint32_t *)depth);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_lidar_depth_splat(int n, const float *points, const float *l2w12, float min_z, float max_depth,
                                     const sgn_seed_cam *cam, float *depth, sgn_stream_t stream) {
    SGN_ARG_CHECK(n >= 1 && n <= SGN_SEED_MAX_POINTS, -1);
    SGN_ARG_CHECK(max_depth > 0.f, -2);
    SGN_ARG_CHECK(cam != nullptr, -4);
    SGN_ARG_CHECK(cam->width >= 1 && cam->width <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(cam->height >= 1 && cam->height <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(points != nullptr, -4);
    SGN_ARG_CHECK(l2w12 != nullptr, -4);
    SGN_ARG_CHECK(depth != nullptr, -4);
    SplatArgs C;
    for (int k = 0; k < 12; ++k) { C.L[k] = l2w12[k]; C.V[k] = cam->w2c[k]; }
    C.fx = cam->fx; C.fy = cam->fy; C.cx = cam->cx; C.cy = cam->cy; C.min_z = min_z; C.max_depth = max_depth;
    C.W = cam->width; C.H = cam->height;
    hipLaunchKernelGGL(depth_splat_kernel, dim3(sgn_cdiv(n, LD_BLOCK)), dim3(LD_BLOCK), 0, (hipStream_t)stream, n, points,
                       C, (uint32_t *)depth);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_lidar_depth_finish(const float *depth, int height, int width, int radius, float rel_tol, float *out,
                                      sgn_stream_t stream) {
    SGN_ARG_CHECK(width >= 1 && width <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(height >= 1 && height <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(radius >= 0 && radius <= SGN_LIDAR_DEPTH_MAX_RADIUS, -2);
    SGN_ARG_CHECK(rel_tol >= 0.f && rel_tol < 1.f, -2);
    SGN_ARG_CHECK(depth != nullptr, -4);
    SGN_ARG_CHECK(out != nullptr, -4);
    SGN_ARG_CHECK(out != depth, -6);
    const float keep = 1.0f - rel_tol;                  // one fp32 subtraction on the host
    hipLaunchKernelGGL(depth_finish_kernel, dim3(sgn_cdiv(width, LD_TILE), sgn_cdiv(height, LD_TILE)),
                       dim3(LD_TILE * LD_TILE), 0, (hipStream_t)stream, height, width, radius, keep, depth, out);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_depth_loss_fwd(int img_h, int img_w, const float *dsum, const float *alpha, const float *target,
                                  const unsigned char *mask, int kind, float *loss_out, int32_t *count_out, void *ws,
                                  size_t ws_bytes, sgn_stream_t stream) {
    SGN_ARG_CHECK(img_w >= 1 && img_w <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(img_h >= 1 && img_h <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(kind == SGN_DEPTH_LOSS_L1 || kind == SGN_DEPTH_LOSS_INVERSE, -2);
    SGN_ARG_CHECK(dsum != nullptr, -4);
    SGN_ARG_CHECK(alpha != nullptr, -4);
    SGN_ARG_CHECK(target != nullptr, -4);
    SGN_ARG_CHECK(loss_out != nullptr, -4);
    SGN_ARG_CHECK(count_out != nullptr, -4);
    SGN_ARG_CHECK(ws != nullptr, -4);
    SGN_ARG_CHECK(ws_bytes >= SGN_DEPTH_LOSS_WS_BYTES, -5);
    hipStream_t s = (hipStream_t)stream;
    const int n_pix = img_h * img_w;
    SGN_HIP_CHECK(hipMemsetAsync(ws, 0, sizeof(LossSums), s));
    sgn_timing_begin(SGN_T_LOSS_FWD, s);
    hipLaunchKernelGGL(depth_loss_fwd_kernel, dim3(sgn_cdiv(n_pix, LD_BLOCK)), dim3(LD_BLOCK), 0, s, n_pix, kind, dsum,
                       alpha, target, mask, (LossSums *)ws);
    hipLaunchKernelGGL(depth_loss_mean_kernel, dim3(1), dim3(1), 0, s, (const LossSums *)ws, loss_out, count_out);
    sgn_timing_end(SGN_T_LOSS_FWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_depth_loss_bwd(int img_h, int img_w, const float *dsum, const float *alpha, const float *target,
                                  const unsigned char *mask, int kind, const float *v_loss, const int32_t *count,
                                  float *v_dsum, float *v_alpha, sgn_stream_t stream) {
    SGN_ARG_CHECK(img_w >= 1 && img_w <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(img_h >= 1 && img_h <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(kind == SGN_DEPTH_LOSS_L1 || kind == SGN_DEPTH_LOSS_INVERSE, -2);
    SGN_ARG_CHECK(dsum != nullptr, -4);
    SGN_ARG_CHECK(alpha != nullptr, -4);
    SGN_ARG_CHECK(target != nullptr, -4);
    SGN_ARG_CHECK(v_loss != nullptr, -4);
    SGN_ARG_CHECK(count != nullptr, -4);
    SGN_ARG_CHECK(v_dsum != nullptr, -4);
    SGN_ARG_CHECK(v_alpha != nullptr, -4);
    hipStream_t s = (hipStream_t)stream;
    const int n_pix = img_h * img_w;
    sgn_timing_begin(SGN_T_LOSS_BWD, s);
    hipLaunchKernelGGL(depth_loss_bwd_kernel, dim3(sgn_cdiv(n_pix, LD_BLOCK)), dim3(LD_BLOCK), 0, s, n_pix, kind, dsum,
                       alpha, target, mask, v_loss, count, v_dsum, v_alpha);
    sgn_timing_end(SGN_T_LOSS_BWD, s);
    SGN_LAUNCH_CHECK();
    return 0;
}

SGN_EXPORT int sgn_depth_metrics(int img_h, int img_w, const float *dsum, const float *alpha, const float *target,
                                 const unsigned char *mask, float *out5, void *ws, size_t ws_bytes,
                                 sgn_stream_t stream) {
    SGN_ARG_CHECK(img_w >= 1 && img_w <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(img_h >= 1 && img_h <= SGN_SEED_MAX_IMAGE_DIM, -3);
    SGN_ARG_CHECK(dsum != nullptr, -4);
    SGN_ARG_CHECK(alpha != nullptr, -4);
    SGN_ARG_CHECK(target != nullptr, -4);
    SGN_ARG_CHECK(out5 != nullptr, -4);
    SGN_ARG_CHECK(ws != nullptr, -4);
    SGN_ARG_CHECK(ws_bytes >= SGN_DEPTH_LOSS_WS_BYTES, -5);
    hipStream_t s = (hipStream_t)stream;
    const int n_pix = img_h * img_w;
    SGN_HIP_CHECK(hipMemsetAsync(ws, 0, sizeof(MetricSums), s));
    hipLaunchKernelGGL(depth_metrics_kernel, dim3(sgn_cdiv(n_pix, LD_BLOCK)), dim3(LD_BLOCK), 0, s, n_pix, dsum, alpha,
                       target, mask, (MetricSums *)ws, out5);
    SGN_LAUNCH_CHECK();
    return 0;
}
