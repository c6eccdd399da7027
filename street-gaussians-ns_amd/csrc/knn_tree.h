// knn_tree.h — the search structure shared by knn.hip (a cloud against itself) and cloud_nn.hip (one cloud against
// another): bounding box, 63-bit Morton keys, sorted points in 64-point leaves and an implicit heap of AABBs, with the
// two distance forms whose operation order makes `box_d2 <= d2` hold bit for bit.  Each including translation unit gets
// its own (internal) copy of the kernels; the pipeline and the exactness argument are described in knn.hip.
#pragma once
#include "sgn_common.h"

namespace {

constexpr int KNN_LEAF = 64;            // points per leaf = lanes per wave
constexpr int KNN_BBOX_BLOCKS = 256;    // partial boxes of the first pass
constexpr int KNN_STACK = 64;           // per-wave LDS stack; depth-first with two pushes per level needs <= levels + 1
constexpr int KNN_QUERY_WAVES = 4;      // waves (leaves) per query block
constexpr int KNN_MAX_N = 1 << 30;      // keeps n * k and the padded point count inside int32 / the sort's range

inline size_t knn_align(size_t b) { return (b + 255) & ~(size_t)255; }

inline int knn_leaves(int n) { return (n + KNN_LEAF - 1) / KNN_LEAF; }
inline int knn_pow2(int l) { int p = 1; while (p < l) p <<= 1; return p; }

struct KnnLayout {
    float *partial;        // [KNN_BBOX_BLOCKS][8]: lo xyz, pad, hi xyz, pad
    int64_t *keys_in, *keys_out;
    int32_t *ids_in, *ids_out;
    float4 *pts;           // [leaves * 64] sorted points, +inf padded
    float4 *nodes;         // [2P][2]: lo, hi
    void *sort_ws;
    size_t sort_ws_bytes, total;
};

KnnLayout knn_layout(int n, void *ws) {
    KnnLayout L{};
    const int leaves = knn_leaves(n), p2 = knn_pow2(leaves);
    char *base = (char *)ws;
    size_t off = 0;
    auto take = [&](size_t b) { char *q = base ? base + off : nullptr; off += knn_align(b); return q; };
    L.partial = (float *)take((size_t)KNN_BBOX_BLOCKS * 8 * sizeof(float));
    L.keys_in = (int64_t *)take((size_t)n * 8);
    L.keys_out = (int64_t *)take((size_t)n * 8);
    L.ids_in = (int32_t *)take((size_t)n * 4);
    L.ids_out = (int32_t *)take((size_t)n * 4);
    L.pts = (float4 *)take((size_t)leaves * KNN_LEAF * sizeof(float4));
    L.nodes = (float4 *)take((size_t)2 * p2 * 2 * sizeof(float4));
    L.sort_ws_bytes = sgn_sort_workspace_bytes(n);
    L.sort_ws = (void *)take(L.sort_ws_bytes);
    L.total = off;
    return L;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// 256 threads, grid-stride over the points; block b writes partial[b]
__global__ __launch_bounds__(256) void knn_bbox_partial(int n, const float *__restrict__ x, float *__restrict__ partial) {
    __shared__ float red[4][6];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = x[(size_t)i * 3 + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    if (lane == 0)
        for (int a = 0; a < 3; ++a) { red[w][a] = lo[a]; red[w][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        float v = red[0][a];
        for (int j = 1; j < 4; ++j) v = a < 3 ? fminf(v, red[j][a]) : fmaxf(v, red[j][a]);
        partial[blockIdx.x * 8 + (a < 3 ? a : a + 1)] = v;
    }
}

// 21 bits -> every third bit of 63
__device__ __forceinline__ uint64_t knn_spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__device__ __forceinline__ uint32_t knn_quant(float v, float lo, float s) {
    const float q = (v - lo) * s;                    // NaN (non-finite input, a caller error) -> cell 0
    if (!(q > 0.f)) return 0u;
    return q >= 2097151.f ? 2097151u : (uint32_t)q;
}

__global__ __launch_bounds__(256) void knn_morton(int n, int nparts, const float *__restrict__ x,
                                                  const float *__restrict__ partial, int64_t *__restrict__ keys,
                                                  int32_t *__restrict__ ids) {
    __shared__ float box[6];
    if (threadIdx.x < 64) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int b = threadIdx.x; b < nparts; b += 64)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], partial[b * 8 + a]);
                hi[a] = fmaxf(hi[a], partial[b * 8 + 4 + a]);
            }
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
        if (threadIdx.x == 0)
            for (int a = 0; a < 3; ++a) { box[a] = lo[a]; box[3 + a] = hi[a]; }
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // one scale for all three axes (cubic cells keep the leaves compact on flat street clouds); extent 0 -> one cell
    const float ext = fmaxf(fmaxf(box[3] - box[0], box[4] - box[1]), box[5] - box[2]);
    const float s = ext > 0.f ? 2097152.f / ext : 0.f;
    const uint32_t qx = knn_quant(x[(size_t)i * 3 + 0], box[0], s);
    const uint32_t qy = knn_quant(x[(size_t)i * 3 + 1], box[1], s);
    const uint32_t qz = knn_quant(x[(size_t)i * 3 + 2], box[2], s);
    keys[i] = (int64_t)(knn_spread3(qx) << 2 | knn_spread3(qy) << 1 | knn_spread3(qz));
    ids[i] = i;
}

__global__ __launch_bounds__(256) void knn_gather(int n, int npad, const float *__restrict__ x,
                                                  const int32_t *__restrict__ ids, float4 *__restrict__ pts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    float4 p = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
    if (i < n) {
        const size_t j = (size_t)ids[i] * 3;
        p = make_float4(x[j], x[j + 1], x[j + 2], 0.f);
    }
    pts[i] = p;
}

// one wave per leaf slot l < P: nodes[P + l] = AABB of its valid points (empty box past the last real leaf)
__global__ __launch_bounds__(256) void knn_leaf_box(int n, int p2, const float4 *__restrict__ pts,
                                                    float4 *__restrict__ nodes) {
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (l >= p2) return;
    const int i = l * KNN_LEAF + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (i < n) {
        const float4 p = pts[i];
        lo = make_float4(p.x, p.y, p.z, 0.f);
        hi = lo;
    }
    lo.x = wave_min(lo.x); lo.y = wave_min(lo.y); lo.z = wave_min(lo.z);
    hi.x = wave_max(hi.x); hi.y = wave_max(hi.y); hi.z = wave_max(hi.z);
    if (lane == 0) {
        nodes[(size_t)(p2 + l) * 2] = lo;
        nodes[(size_t)(p2 + l) * 2 + 1] = hi;
    }
}

// nodes [first, 2 * first): union of their two children
__global__ __launch_bounds__(256) void knn_level_box(int first, float4 *__restrict__ nodes) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= first) return;
    const int v = first + t;
    const float4 al = nodes[(size_t)(2 * v) * 2], ah = nodes[(size_t)(2 * v) * 2 + 1];
    const float4 bl = nodes[(size_t)(2 * v + 1) * 2], bh = nodes[(size_t)(2 * v + 1) * 2 + 1];
    nodes[(size_t)v * 2] = make_float4(fminf(al.x, bl.x), fminf(al.y, bl.y), fminf(al.z, bl.z), 0.f);
    nodes[(size_t)v * 2 + 1] = make_float4(fmaxf(ah.x, bh.x), fmaxf(ah.y, bh.y), fmaxf(ah.z, bh.z), 0.f);
}

__device__ __forceinline__ float knn_d2(float qx, float qy, float qz, float px, float py, float pz) {
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

// squared distance from q to the box [lo, hi]: per-axis gap max(lo - q, 0, q - hi), summed like knn_d2
__device__ __forceinline__ float knn_box_d2(float qx, float qy, float qz, float4 lo, float4 hi) {
    const float gx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

// Queues the whole build over points [n,3] into L on `stream`: L.keys_out / L.ids_out hold the sorted keys and ids,
// L.pts the padded leaves, L.nodes the heap (root 1, leaves at p2 + l).  L.partial keeps the partial boxes (*nparts of
// them), from which knn_morton can key another cloud on the same cube.
inline int knn_build_tree(int n, const float *points, const KnnLayout &L, int *nparts_out, sgn_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    const int leaves = knn_leaves(n), p2 = knn_pow2(leaves), npad = leaves * KNN_LEAF;
    const int nparts = sgn_cdiv(n, 256) < KNN_BBOX_BLOCKS ? sgn_cdiv(n, 256) : KNN_BBOX_BLOCKS;
    if (nparts_out) *nparts_out = nparts;

    hipLaunchKernelGGL(knn_bbox_partial, dim3(nparts), dim3(256), 0, s, n, points, L.partial);
    hipLaunchKernelGGL(knn_morton, dim3(sgn_cdiv(n, 256)), dim3(256), 0, s, n, nparts, points, L.partial, L.keys_in,
                       L.ids_in);
    SGN_LAUNCH_CHECK();
    const int rc = sgn_sort_pairs(n, 0, 63, L.keys_in, L.ids_in, L.keys_out, L.ids_out, L.sort_ws, L.sort_ws_bytes,
                                  /*documented ballot ranking*/ 0, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(knn_gather, dim3(sgn_cdiv(npad, 256)), dim3(256), 0, s, n, npad, points, L.ids_out, L.pts);
    hipLaunchKernelGGL(knn_leaf_box, dim3(sgn_cdiv(p2, 4)), dim3(256), 0, s, n, p2, L.pts, L.nodes);
    for (int first = p2 >> 1; first >= 1; first >>= 1)
        hipLaunchKernelGGL(knn_level_box, dim3(sgn_cdiv(first, 256)), dim3(256), 0, s, first, L.nodes);
    SGN_LAUNCH_CHECK();
    return 0;
}

}  // namespace
