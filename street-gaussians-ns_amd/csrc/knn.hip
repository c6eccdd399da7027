// knn.hip — exact k-nearest-neighbour search over 3-D points (gfx950), for the initial Gaussian scales.
//
// Replaces sklearn's NearestNeighbors(k+1).kneighbors(x)[:, 1:] as the reference uses it in
// SplatfactoModel.populate_modules (street_gaussians_ns/sgn_splatfacto.py:260-264, k_nearest_sklearn :439-457):
// for every point the k smallest |x_i - x_j| over j != i, ascending, with their j.
//
// Pipeline (all on `stream`, no host synchronisation):
//   knn_bbox_partial   per-block AABB of the points                      -> partial[KNN_BBOX_BLOCKS]
//   knn_morton         every block folds the partial boxes, then one 63-bit Morton key per point (21 bits per axis
//                      over the cube of the largest extent: with 10 bits a far outlier collapses the dense core)
//   sgn_sort_pairs     (key, id) over bits [0, 63), stable, documented ballot ranking (radix_sort.hip)
//   knn_gather         sorted points as float4, padded to whole 64-point leaves with +inf points
//   knn_leaf_box       one wave per leaf: the AABB of its valid points (empty leaves of the power-of-two padding: an
//                      empty box, +inf lower / -inf upper corner, whose distance to anything is +inf)
//   knn_level_box      one launch per tree level: implicit heap (root 1, leaves at P + l), parent = union of children
//   knn_query<K>       one wave per leaf of 64 queries: own leaf first, then a depth-first walk with a wave-uniform
//                      stack in LDS, entering a node only if ballot(box_d2 < kth_d2) is non-zero; a leaf's 64 candidates
//                      are read with wave-uniform (scalar) loads and tested against every lane.
//
// Exactness.  Distances are fp32 direct differences, d2 = (dx*dx + dy*dy) + dz*dz (no FMA: -ffp-contract=off), and a
// box's distance is formed the same way from the per-axis gaps, which are fp-monotone in the point: for every point p
// inside a box B, box_d2(q, B) <= d2(q, p) holds bit for bit, so pruning on `box_d2 < kth_d2` never drops a candidate
// that the insertion test `d2 < kth_d2` would have kept.  The kept set is therefore k smallest fp32 d2 over j != i.
// Both tests are strict: a node or candidate that only ties the current k-th distance is skipped, which bounds the work
// on duplicates and lattices (all points identical: the own leaf alone, 64 candidates per query).
//
// Determinism.  The traversal order is a function of the sorted input alone and the top-k insertion keeps the first
// of equal distances in visit order, so results are bit-identical run to run; the only atomic is the optional
// `visited` counter (a sum).
//
// Top-k: K slots in registers with K a compile-time bucket (1, 2, 4, 8, 16).  For k < K the first K - k slots are
// sentinels at d2 = -1 that no candidate displaces, so the k-th distance is always slot K - 1 and every index into the
// arrays is static (ScratchSize 0).
#include "sgn_common.h"

#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "knn.hip is written for gfx950 (MI355X) only"
#endif

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

template <int K>
struct TopK {
    float d[K];
    int j[K];
    // strict: a candidate equal to a kept distance goes behind it (the first of equal distances stays first).  Every
    // slot is computed from the old values only: shift down from the slot above, take the candidate, or keep.
    __device__ __forceinline__ void insert(float cd, int cj) {
#pragma unroll
        for (int s = K - 1; s > 0; --s) {
            const bool shift = cd < d[s - 1], here = cd < d[s];
            d[s] = shift ? d[s - 1] : here ? cd : d[s];
            j[s] = shift ? j[s - 1] : here ? cj : j[s];
        }
        const bool first = cd < d[0];
        d[0] = first ? cd : d[0];
        j[0] = first ? cj : j[0];
    }
};

// all 64 candidates of leaf `leaf` against this lane's query (sorted index self); wave-uniform addresses -> scalar loads
template <int K>
__device__ __forceinline__ void knn_scan_leaf(const float4 *__restrict__ pts, int leaf, float qx, float qy, float qz,
                                              int self, TopK<K> &top) {
    const int base = leaf * KNN_LEAF;
    const float4 *c = pts + base;
#pragma unroll 4
    for (int t = 0; t < KNN_LEAF; ++t) {
        const float4 p = c[t];
        const float d2 = knn_d2(qx, qy, qz, p.x, p.y, p.z);
        if (d2 < top.d[K - 1] && base + t != self) top.insert(d2, base + t);
    }
}

template <int K>
__global__ __launch_bounds__(64 * KNN_QUERY_WAVES) void knn_query(int n, int k, int leaves, int p2,
                                                                  const float4 *__restrict__ pts,
                                                                  const float4 *__restrict__ nodes,
                                                                  const int32_t *__restrict__ ids,
                                                                  float *__restrict__ dist, int32_t *__restrict__ idx,
                                                                  unsigned long long *__restrict__ visited) {
    __shared__ int stack_lds[KNN_QUERY_WAVES][KNN_STACK];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int leaf = __builtin_amdgcn_readfirstlane(blockIdx.x * KNN_QUERY_WAVES + w);
    if (leaf >= leaves) return;
    int *stack = stack_lds[w];
    const int self = leaf * KNN_LEAF + lane;
    const bool valid = self < n;
    const float4 q = pts[self];
    TopK<K> top;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        top.d[s] = s < K - k ? -1.f : INFINITY;   // sentinels below every real distance: the k-th is slot K - 1
        top.j[s] = -1;
    }
    const unsigned long long nvalid = __popcll(__ballot(valid));
    unsigned long long nleaf = 1;
    knn_scan_leaf<K>(pts, leaf, q.x, q.y, q.z, self, top);

    const int own = p2 + leaf;
    int sp = 0;
    if (own != 1) {                       // (a tree of one leaf: nothing else to visit)
        stack[0] = 1;
        sp = 1;
    }
    while (sp > 0) {
        --sp;
        const int v = __builtin_amdgcn_readfirstlane(stack[sp]);
        const float4 lo = nodes[(size_t)v * 2], hi = nodes[(size_t)v * 2 + 1];
        const float bd2 = knn_box_d2(q.x, q.y, q.z, lo, hi);
        if (__ballot(valid && bd2 < top.d[K - 1]) == 0) continue;
        if (v >= p2) {
            knn_scan_leaf<K>(pts, v - p2, q.x, q.y, q.z, self, top);
            ++nleaf;
            continue;
        }
        // children of v cover leaves [lo_leaf, lo_leaf + span); the half holding (or nearer in Morton order to) the
        // wave's own leaf is popped first.  The own leaf itself is never pushed.
        const int lvl = 31 - __builtin_clz(v);                       // depth of v
        const int span = p2 >> (lvl + 1);                            // leaves under each child
        const int mid = (v << (31 - __builtin_clz(p2) - lvl)) - p2 + span;
        const int cl = 2 * v, cr = 2 * v + 1;
        const int first = leaf < mid ? cl : cr, second = leaf < mid ? cr : cl;
        // at most one pending sibling per level plus the pair just pushed: <= levels + 1 < KNN_STACK entries.  Every
        // lane stores the same value, so each lane's later read follows its own store in program order.
        if (second != own) stack[sp++] = second;
        if (first != own) stack[sp++] = first;
    }

    if (visited && lane == 0) atomicAdd(visited, nleaf * KNN_LEAF * nvalid);
    if (!valid) return;
    const size_t row = (size_t)ids[self] * k;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        if (s >= K - k) {
            dist[row + s - (K - k)] = sqrtf(top.d[s]);
            idx[row + s - (K - k)] = top.j[s] >= 0 ? ids[top.j[s]] : -1;   // (-1 only for non-finite input)
        }
    }
}

template <int K>
void knn_query_launch(int n, int k, int leaves, int p2, const KnnLayout &L, float *dist, int32_t *idx,
                      int64_t *visited, hipStream_t s) {
    hipLaunchKernelGGL(knn_query<K>, dim3(sgn_cdiv(leaves, KNN_QUERY_WAVES)), dim3(64 * KNN_QUERY_WAVES), 0, s, n, k,
                       leaves, p2, L.pts, L.nodes, L.ids_out, dist, idx, (unsigned long long *)visited);
}

}  // namespace

SGN_EXPORT size_t sgn_knn_workspace_bytes(int n, int k) {
    (void)k;
    if (n <= 0 || n > KNN_MAX_N) return 0;
    return knn_layout(n, nullptr).total;
}

SGN_EXPORT int sgn_knn(int n, int k, const float *points, float *dist, int32_t *idx, int64_t *visited, void *ws,
                       size_t ws_bytes, sgn_stream_t stream) {
    SGN_ARG_CHECK(k >= 1 && k <= 16, -1);
    SGN_ARG_CHECK(n > k && n <= KNN_MAX_N, -2);
    SGN_ARG_CHECK(points && dist && idx && ws, -3);
    SGN_ARG_CHECK(ws_bytes >= sgn_knn_workspace_bytes(n, k), -4);
    hipStream_t s = (hipStream_t)stream;
    const KnnLayout L = knn_layout(n, ws);
    const int leaves = knn_leaves(n), p2 = knn_pow2(leaves), npad = leaves * KNN_LEAF;
    const int nparts = sgn_cdiv(n, 256) < KNN_BBOX_BLOCKS ? sgn_cdiv(n, 256) : KNN_BBOX_BLOCKS;

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
    switch (k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16) {
        case 1: knn_query_launch<1>(n, k, leaves, p2, L, dist, idx, visited, s); break;
        case 2: knn_query_launch<2>(n, k, leaves, p2, L, dist, idx, visited, s); break;
        case 4: knn_query_launch<4>(n, k, leaves, p2, L, dist, idx, visited, s); break;
        case 8: knn_query_launch<8>(n, k, leaves, p2, L, dist, idx, visited, s); break;
        default: knn_query_launch<16>(n, k, leaves, p2, L, dist, idx, visited, s); break;
    }
    SGN_LAUNCH_CHECK();
    return 0;
}
